#!/usr/bin/env python3
"""Weighted pooled pull and push of the row-sharded store (ShardedEmbedding.pull_wsum / push_wbags) against the composed
sequences they replace, at world size 1 on the full Criteo-sized table.  Method and helpers are tools/shard_bag_bench.py's: one
process, variants alternating, every variant warmed, median / minimum / maximum over `--reps` windows.

Per shape (B, F, d) and dead share (0 %, 50 %, 85 %: synthetic -- the ids are herald_amd.synth.criteo_batch's, the dead
occurrences are drawn uniformly, carry weight 0 and name the padding id 0, as tools/wbag_bench.py builds them; nobody has measured
the reference's datasets here):

  kernel pairs -- `--iters` calls over `--distinct` batches captured into one device graph per window (plans and the unique rows
  of every batch are prepared before the timed windows):
    pull   expand_wsum         ha_gather_wsum_u32keys over the received unique rows and the plan's inverse
           expand+wsum         ha_gather_u32keys to [n, d], then ha_gather_wsum_* over the positions 0 .. n-1
    push   reduce_wbags        ha_dedup_reduce_wbags on the pooled gradient [B, d]
           grad_rows+reduce    ha_wbag_grad_rows to [n, d], then ha_dedup_reduce_scaled
           reduce_wbags/spread (85 % only) ha_dedup_reduce_wbags on the same batches with every dead slot folded onto an id of
                               its own instead of id 0: the same live work without key 0's all-dead run -- the difference is
                               what that run costs the reduce launch

  whole calls -- plain launches (a call reads its routing counts back on the host), `--call-iters` calls per window, host
  clock around the window, which a device synchronise closes:
    step   pull_wsum+push_wbags        pull_wsum(ids, w) and push_wbags of the same route
           pull+wsum+grad_rows+push    pull(ids), the weighted sum over the rows, the expanded gradient, push of the same route

The yardstick is always the composed sequence, in the same process.  The condition reported is bag_bench's: fused <= composed, a
difference within the larger of the two variants' own window spreads counting as equal.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from bag_bench import init_table, time_variants, verdict
from shard_bag_bench import time_calls
from herald_amd import ops, synth
from herald_amd.sharded import ShardedEmbedding

DEAD = {"dead0": 0.0, "dead50": 0.5, "dead85": 0.85}


def summarise(times):
    return {name: {"median_us": float(np.median(ts)), "min_us": float(min(ts)), "max_us": float(max(ts)), "windows": len(ts)}
            for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x128,256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--dead", default="dead0,dead50,dead85", help="dead shares, comma separated: " + ", ".join(DEAD))
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=200, help="calls per graph-captured window (kernel pairs)")
    ap.add_argument("--call-iters", type=int, default=50, help="calls per plain-launch window (whole calls)")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shard_wbag_bench.py measures on the GPU; there is none here")
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
        raw = [synth.as_f32_ids(synth.criteo_batch(B, step=s, rows=args.rows, nfields=F)) for s in range(args.distinct)]
        pos = torch.arange(n, dtype=torch.int64, device=dev).view(B, F)
        pooled = torch.empty((B, d), dtype=torch.float32, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        bag_grads = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen)
        scale = -args.lr
        for dead in args.dead.split(","):
            rng = np.random.default_rng(789)
            host_w = [(rng.random(h.shape) >= DEAD[dead]).astype(np.float32) for h in raw]
            host = [np.where(w != 0, h, np.float32(0)) for h, w in zip(raw, host_w)]
            longest = int(max(np.unique(h, return_counts=True)[1].max() for h in host))
            U = float(np.mean([np.unique(h).size for h in host]))
            ids = [torch.from_numpy(h).to(dev) for h in host]
            ws = [torch.from_numpy(w).to(dev) for w in host_w]
            nd = len(ids)
            plans = [ops.IndexPlan(n, dev).build(t.reshape(-1), key_limit=args.rows) for t in ids]
            rows_u = [eng.gather_keys(table, p.uniq()) for p in plans]

            def expand_wsum(i):
                eng.expand_wsum(rows_u[i % nd], plans[i % nd], ws[i % nd], bag=F, out=pooled)

            def expand_then_wsum(i):
                rows = eng.expand(rows_u[i % nd], plans[i % nd])
                ops.embedding_lookup_wsum(rows, pos, ws[i % nd], out=pooled)

            def reduce_wbags(i):
                eng.reduce_scaled_wbags(plans[i % nd], bag_grads, ws[i % nd], scale, bag=F)

            def grad_rows_then_reduce(i):
                eng.reduce_scaled(plans[i % nd], ops.wbag_grad_rows(bag_grads, ws[i % nd].view(-1), bag=F), scale)

            pull = summarise(time_variants({"expand_wsum": expand_wsum, "expand+wsum": expand_then_wsum}, args.reps,
                                           args.iters, True, dev))
            push_variants = {"reduce_wbags": reduce_wbags, "grad_rows+reduce": grad_rows_then_reduce}
            if dead == "dead85":
                # every dead slot on an id of its own (the table's last rows, none of them drawn by a 256 .. 4,096 batch's
                # live slots with any likelihood): the live work is the same, key 0's all-dead run is gone
                top = min(args.rows, 1 << 24) - 1       # (float32 ids: every integer up to 2^24 is representable)
                spread = [np.where(w != 0, h, (top - np.arange(h.size).reshape(h.shape)).astype(np.float32))
                          for h, w in zip(raw, host_w)]
                plans_s = [ops.IndexPlan(n, dev).build(torch.from_numpy(h).to(dev).reshape(-1), key_limit=args.rows)
                           for h in spread]

                def reduce_wbags_spread(i):
                    eng.reduce_scaled_wbags(plans_s[i % nd], bag_grads, ws[i % nd], scale, bag=F)

                push_variants["reduce_wbags/spread"] = reduce_wbags_spread
            push = summarise(time_variants(push_variants, args.reps, args.iters, True, dev))

            def fused_step(i):
                _, r = emb.pull_wsum(ids[i % nd], ws[i % nd], return_route=True, out=pooled)
                emb.push_wbags(None, bag_grads, ws[i % nd], args.lr, route=r)

            def composed_step(i):
                rows, r = emb.pull(ids[i % nd], return_route=True)
                ops.embedding_lookup_wsum(rows.view(n, d), pos, ws[i % nd], out=pooled)
                emb.push(None, ops.wbag_grad_rows(bag_grads, ws[i % nd].view(-1), bag=F), args.lr, route=r)

            step = summarise(time_calls({"pull_wsum+push_wbags": fused_step, "pull+wsum+grad_rows+push": composed_step},
                                        args.reps, args.call_iters, dev))
            entry = {"n": n, "dead_share": DEAD[dead], "mean_unique": U, "longest_run": longest, "pull": pull, "push": push,
                     "step": step,
                     "conditions": {"expand_wsum<=expand+wsum": verdict(pull, "expand_wsum", "expand+wsum"),
                                    "reduce_wbags<=grad_rows+reduce": verdict(push, "reduce_wbags", "grad_rows+reduce"),
                                    "pull_wsum+push_wbags<=composed": verdict(step, "pull_wsum+push_wbags",
                                                                              "pull+wsum+grad_rows+push")}}
            if "reduce_wbags/spread" in push:
                entry["all_dead_run_us"] = push["reduce_wbags"]["median_us"] - push["reduce_wbags/spread"]["median_us"]
            results["shapes"]["%dx%dx%d/%s" % (B, F, d, dead)] = entry
            print("== B=%d F=%d d=%d %s  n=%d  mean unique %.0f  longest run %d" % (B, F, d, dead, n, U, longest))
            for side in ("pull", "push", "step"):
                for name, r in entry[side].items():
                    print("  %-5s %-25s median %8.2f us  [%7.2f .. %7.2f]" % (side, name, r["median_us"], r["min_us"],
                                                                             r["max_us"]))
            for name, v in entry["conditions"].items():
                print("  condition %-32s %s  (difference %+.2f us, spread %.2f us)" % (
                    name, "met" if v["met"] else "MISSED", v["a_minus_b_us"], v["spread_us"]))
            if "all_dead_run_us" in entry:
                print("  key 0's all-dead run costs the reduce launch %+.2f us (medians)" % entry["all_dead_run_us"])
            sys.stdout.flush()
            del plans, rows_u
        del emb
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
