#!/usr/bin/env python3
"""Sum-pooled pull and push of the row-sharded store (ShardedEmbedding.pull_sum / push_bags) against the unfused sequences
they replace, at world size 1 on the full Criteo-sized table.  Method and helpers are tools/bag_bench.py's: one process,
variants alternating, every variant warmed, median / minimum / maximum over `--reps` windows, algorithmic bytes (from the
shapes and the batches' unique counts, below) over the median.

Per shape (B, F, d):

  kernel pairs -- `--iters` calls over `--distinct` batches captured into one device graph per window (plans and the unique rows
  of every batch are prepared before the timed windows):
    pull   expand_sum          ha_gather_sum_u32keys over the received unique rows and the plan's inverse
           expand+sum          ha_gather_u32keys to [n, d], then ha_gather_sum_* over the positions 0 .. n-1
    push   reduce_bags         ha_dedup_reduce_bags on the pooled gradient [B, d]
           expanded+reduce     IndexedSlices.expanded_values (a gather to [n, d]), then ha_dedup_reduce_scaled

  whole calls -- plain launches (a call reads its routing counts back on the host), `--call-iters` calls per window, host
  clock around the window, which a device synchronise closes (time_calls below: whatever stream the store used):
    step   pull_sum+push_bags  pull_sum(ids) and push_bags of the same route
           pull+sum+expand+push  pull(ids), the sum over the rows, the expanded gradient, push of the same route

The yardstick is always the unfused sequence, in the same process.  The condition reported per shape is bag_bench's: fused <=
unfused, a difference within the larger of the two variants' own window spreads counting as equal.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from bag_bench import init_table, summarise, time_variants, verdict
from herald_amd import ops, synth
from herald_amd.sharded import ShardedEmbedding


def pair_bytes(B, F, d, U):
    n = B * F
    return {"expand_sum": U * 4 * d + n * 4 + B * 4 * d,                       # unique rows, inverse, pooled rows
            # ... the rows written per occurrence, read back with their positions (int64), summed
            "expand+sum": U * 4 * d + n * 4 + n * 4 * d + n * (4 * d + 8) + B * 4 * d,
            "reduce_bags": n * 8 + B * 4 * d + U * 4 * d,                      # sorted keys + occurrence indices, bag rows, reduced
            # ... the bag rows gathered to [n, d] through an int64 index, read back
            "expanded+reduce": B * 4 * d + n * 8 + n * 4 * d + n * 8 + n * 4 * d + U * 4 * d}


def step_bytes(B, F, d, U):
    """A pull and a push of one batch at world size 1: plan (ids read, ~6 words per id written and read), owner gather and
    the self-exchange copy of U rows each way, the owner's apply (U rows read, added, written), plus the two end steps."""
    n = B * F
    pb = pair_bytes(B, F, d, U)
    common = n * 4 + n * 48 + 2 * (U * (4 + 8 * d) + U * 8 * d) + U * 4 * d
    return {"pull_sum+push_bags": common + pb["expand_sum"] + pb["reduce_bags"],
            "pull+sum+expand+push": common + pb["expand+sum"] + pb["expanded+reduce"]}


def time_calls(variants, reps, iters, dev):
    """time_variants for plain launches, by the host clock around a window that starts and ends with a DEVICE synchronise;
    -> {name: [microseconds per call, one per window]}."""
    for f in variants.values():
        for i in range(min(iters, 8)):                  # warm-up: code objects, allocator, routing workspaces
            f(i)
    torch.cuda.synchronize(dev)
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, f in variants.items():                # alternating
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(iters):
                f(i)
            torch.cuda.synchronize(dev)                 # every stream of the device: whatever the store used
            times[name].append(1e6 * (time.perf_counter() - t0) / iters)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=200, help="calls per graph-captured window (kernel pairs)")
    ap.add_argument("--call-iters", type=int, default=50, help="calls per plain-launch window (whole calls)")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shard_bag_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    results = {"rows": args.rows, "reps": args.reps, "iters": args.iters, "call_iters": args.call_iters,
               "distinct": args.distinct, "device": torch.cuda.get_device_name(dev), "shapes": {}}
    table, table_d = None, None
    for (B, F, d) in shapes:
        if table_d != d:
            table = None
            torch.cuda.empty_cache()
            table, table_d = init_table(args.rows, d, dev), d
        n = B * F
        emb = ShardedEmbedding(args.rows, d, dev, table=table, max_ids=n)
        eng = emb.engine
        host = [synth.as_f32_ids(synth.criteo_batch(B, step=s, rows=args.rows, nfields=F)) for s in range(args.distinct)]
        U = float(np.mean([np.unique(h).size for h in host]))
        ids = [torch.from_numpy(h).to(dev) for h in host]
        nd = len(ids)
        # ---- kernel pairs: plans and the unique rows a pull would have received, prepared untimed
        plans = [ops.IndexPlan(n, dev).build(t.reshape(-1), key_limit=args.rows) for t in ids]
        rows_u = [eng.gather_keys(table, p.uniq()) for p in plans]
        pos = torch.arange(n, dtype=torch.int64, device=dev).view(B, F)
        pooled = torch.empty((B, d), dtype=torch.float32, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        bag_grads = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen)
        scale = -args.lr

        def expand_sum(i):
            eng.expand_sum(rows_u[i % nd], plans[i % nd], bag=F, out=pooled)

        def expand_then_sum(i):
            rows = eng.expand(rows_u[i % nd], plans[i % nd])
            ops.embedding_lookup_sum(rows, pos, out=pooled)

        def reduce_bags(i):
            eng.reduce_scaled_bags(plans[i % nd], bag_grads, scale, bag=F)

        def expanded_then_reduce(i):
            sl = ops.IndexedSlices(indices=ids[i % nd], values=bag_grads, bag=F)
            eng.reduce_scaled(plans[i % nd], sl.expanded_values(), scale)

        pb = pair_bytes(B, F, d, U)
        pull = summarise(time_variants({"expand_sum": expand_sum, "expand+sum": expand_then_sum}, args.reps, args.iters,
                                       True, dev), pb)
        push = summarise(time_variants({"reduce_bags": reduce_bags, "expanded+reduce": expanded_then_reduce}, args.reps,
                                       args.iters, True, dev), pb)

        # ---- whole calls: plain launches, one route per batch shared by its pull and its push
        def fused_step(i):
            _, r = emb.pull_sum(ids[i % nd], return_route=True, out=pooled)
            emb.push_bags(None, bag_grads, args.lr, route=r)

        def unfused_step(i):
            rows, r = emb.pull(ids[i % nd], return_route=True)
            ops.embedding_lookup_sum(rows.view(n, d), pos, out=pooled)
            sl = ops.IndexedSlices(indices=ids[i % nd], values=bag_grads, bag=F)
            emb.push(None, sl.expanded_values(), args.lr, route=r)

        step = summarise(time_calls({"pull_sum+push_bags": fused_step, "pull+sum+expand+push": unfused_step}, args.reps,
                                    args.call_iters, dev), step_bytes(B, F, d, U))
        entry = {"n": n, "mean_unique": U, "pull": pull, "push": push, "step": step,
                 "conditions": {"expand_sum<=expand+sum": verdict(pull, "expand_sum", "expand+sum"),
                                "reduce_bags<=expanded+reduce": verdict(push, "reduce_bags", "expanded+reduce"),
                                "pull_sum+push_bags<=unfused": verdict(step, "pull_sum+push_bags", "pull+sum+expand+push")}}
        results["shapes"]["%dx%dx%d" % (B, F, d)] = entry
        print("== B=%d F=%d d=%d  n=%d  mean unique %.0f" % (B, F, d, n, U))
        for side in ("pull", "push", "step"):
            for name, r in entry[side].items():
                print("  %-5s %-21s median %8.2f us  [%7.2f .. %7.2f]  %6.2f MB  %7.1f GB/s" % (
                    side, name, r["median_us"], r["min_us"], r["max_us"], r["bytes"] / 1e6, r["GBps_at_median"]))
        for name, v in entry["conditions"].items():
            print("  condition %-30s %s  (difference %+.2f us, spread %.2f us)" % (name, "met" if v["met"] else "MISSED",
                                                                                  v["a_minus_b_us"], v["spread_us"]))
        sys.stdout.flush()
        del plans, rows_u, emb
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
