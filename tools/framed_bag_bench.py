#!/usr/bin/env python3
"""Sum-pooled steps of the sharded table's framed step engine (FramedStep.steps_bags, one native call per run of steps) against
what a pooled model pays without them, at world size 1 in one process on the full Criteo-sized table.

Per shape (B, F, d), three drivers over the same store and the same stream of batches, every one a FramedStep of its own:

    steps_bags              pooled pull and pooled push: ha_shard_steps_bags
    steps                   (a) the unpooled native step alone (rows [n, d] out, gradients [n, d] in): ha_shard_steps
    steps+sum+expand        (b) the unpooled native step + embedding_lookup_sum over the delivered rows + the expansion of the
                            pooled gradient [B, d] to [n, d] (IndexedSlices.expanded_values) -- what a pooled model pays today

A window is `--blocks` routing blocks of `--block` steps each, timed by the host clock between two device synchronisations;
the drivers alternate window by window; median [min .. max] of `--reps` windows per line.  The claim to support is
"steps_bags is faster than (b) by more than the spread of the windows"; steps_bags against (a) is reported the same way.
`--profile N`: no timing, N blocks of each driver one after the other (for a kernel trace of the end launches)."""
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

from bag_bench import init_table
from herald_amd import ops, synth
from herald_amd.sharded import FramedStep, ShardedEmbedding


def step_bytes(B, F, d, U):
    """Algorithmic bytes of one step's END launches at world size 1 (the routing is the same in every driver)."""
    n = B * F
    pooled = n * 4 + U * 4 * d + B * 4 * d + n * 8 + B * 4 * d + U * 8 * d
    unpooled = n * 4 + U * 4 * d + n * 4 * d + n * 8 + n * 4 * d + U * 8 * d
    extra = n * (4 * d + 8) + B * 4 * d + B * 4 * d + n * 8 + n * 4 * d      # rows read back and summed; the gradient expanded
    return {"steps_bags": pooled, "steps": unpooled, "steps+sum+expand": unpooled + extra}


class Driver:
    """One FramedStep walking the stream of batches block by block."""

    def __init__(self, kind, emb, ids, B, F, block, lr, bag_grads):
        self.kind, self.ids, self.B, self.F, self.lr = kind, ids, B, F, lr
        n, d, dev = B * F, emb.width, emb.table.device
        self.fs = FramedStep(emb, n, block=block, graphs=False)
        if not self.fs.native_ok():
            raise SystemExit("framed_bag_bench.py: the native step is not available")
        self.nb, self.LA, self.block, self.k = len(ids), self.fs.LOOKAHEAD, block, 0
        pooled = kind == "steps_bags"
        self.staged = [t.view(B, F) if pooled else t.view(-1) for t in ids]
        self.bag_grads = bag_grads
        self.outs = [torch.empty((B, d) if pooled else (n, d), dtype=torch.float32, device=dev) for _ in range(block)]
        if kind == "steps":
            gen = torch.Generator(device=dev)
            gen.manual_seed(789)
            self.grads = [torch.randn((n, d), dtype=torch.float32, device=dev, generator=gen) for _ in range(2)]
        if kind == "steps+sum+expand":
            self.pos = torch.arange(n, dtype=torch.int64, device=dev).view(B, F)
            self.pooled = torch.empty((B, d), dtype=torch.float32, device=dev)
        self.fs.start([self.staged[j % self.nb] for j in range(self.LA)])

    def block_of_steps(self):
        k, cnt, nb, LA = self.k, self.block, self.nb, self.LA
        ahead = [self.staged[(k + i + LA) % nb] for i in range(cnt)]
        if self.kind == "steps_bags":
            self.fs.steps_bags(ahead, [self.bag_grads[(k + i) % 2] for i in range(cnt)], self.lr, outs=self.outs)
        elif self.kind == "steps":
            self.fs.steps(ahead, [self.grads[(k + i) % 2] for i in range(cnt)], self.lr, outs=self.outs)
        else:
            # (the loop holds a batch's gradient when it asks for its rows, as bench.py's does: the expansion comes first)
            grads = [ops.IndexedSlices(indices=self.ids[(k + i) % nb], values=self.bag_grads[(k + i) % 2], bag=self.F)
                     .expanded_values() for i in range(cnt)]
            self.fs.steps(ahead, grads, self.lr, outs=self.outs)
            for o in self.outs:
                ops.embedding_lookup_sum(o, self.pos, out=self.pooled)
        self.k = k + cnt


def verdict(res, a, b):
    """a faster than b by more than the larger of the two spreads?"""
    spread = max(res[a]["max_us"] - res[a]["min_us"], res[b]["max_us"] - res[b]["min_us"])
    diff = res[b]["median_us"] - res[a]["median_us"]
    return {"a": a, "b": b, "b_minus_a_us": diff, "spread_us": spread, "faster_by_more_than_spread": bool(diff > spread),
            "slower_by_more_than_spread": bool(-diff > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=7, help="timed windows per driver")
    ap.add_argument("--block", type=int, default=16, help="steps per routing block (one native call each)")
    ap.add_argument("--blocks", type=int, default=8, help="routing blocks per window")
    ap.add_argument("--distinct", type=int, default=64, help="different batches cycled through")
    ap.add_argument("--lr", type=float, default=1e-6)
    ap.add_argument("--tolerance", type=int, default=1, help="ha_set_tolerance_mode (1 = the sharded bench's setting)")
    ap.add_argument("--profile", type=int, default=0, help="no timing: this many blocks of each driver, one after the other")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("framed_bag_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    prev = ops.set_tolerance_mode(args.tolerance)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    results = {"rows": args.rows, "reps": args.reps, "block": args.block, "blocks": args.blocks, "distinct": args.distinct,
               "tolerance_mode": args.tolerance, "device": torch.cuda.get_device_name(dev), "shapes": {}}
    names = ("steps_bags", "steps", "steps+sum+expand")
    table, table_d = None, None
    try:
        for (B, F, d) in shapes:
            if table_d != d:
                table = None
                torch.cuda.empty_cache()
                table, table_d = init_table(args.rows, d, dev), d
            n = B * F
            emb = ShardedEmbedding(args.rows, d, dev, table=table, max_ids=n)
            host = [synth.as_f32_ids(synth.criteo_batch(B, step=s, rows=args.rows, nfields=F)) for s in range(args.distinct)]
            U = float(np.mean([np.unique(h).size for h in host]))
            ids = [torch.from_numpy(h).to(dev).reshape(-1) for h in host]
            gen = torch.Generator(device=dev)
            gen.manual_seed(456)
            bag_grads = [torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen) for _ in range(2)]
            drivers = {name: Driver(name, emb, ids, B, F, args.block, args.lr, bag_grads) for name in names}
            for drv in drivers.values():                    # warm-up: code objects, allocator, three routing blocks each
                for _ in range(3):
                    drv.block_of_steps()
            torch.cuda.synchronize(dev)
            if args.profile:
                for drv in drivers.values():
                    for _ in range(args.profile):
                        drv.block_of_steps()
                    torch.cuda.synchronize(dev)
                continue
            times = {name: [] for name in names}
            steps = args.block * args.blocks
            for _ in range(args.reps):
                for name, drv in drivers.items():           # alternating
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(args.blocks):
                        drv.block_of_steps()
                    torch.cuda.synchronize(dev)
                    times[name].append(1e6 * (time.perf_counter() - t0) / steps)
            nbytes = step_bytes(B, F, d, U)
            res = {name: {"median_us": float(np.median(ts)), "min_us": float(min(ts)), "max_us": float(max(ts)),
                          "windows": len(ts), "end_launch_bytes": int(nbytes[name])} for name, ts in times.items()}
            entry = {"n": n, "mean_unique": U, "step": res,
                     "vs_unpooled_plus_sum_and_expand": verdict(res, "steps_bags", "steps+sum+expand"),
                     "vs_unpooled_alone": verdict(res, "steps_bags", "steps")}
            results["shapes"]["%dx%dx%d" % (B, F, d)] = entry
            print("== B=%d F=%d d=%d  n=%d  mean unique %.0f" % (B, F, d, n, U))
            for name in names:
                r = res[name]
                print("  %-18s median %8.2f us per step  [%7.2f .. %7.2f]  end launches %6.2f MB" % (
                    name, r["median_us"], r["min_us"], r["max_us"], r["end_launch_bytes"] / 1e6))
            for key in ("vs_unpooled_plus_sum_and_expand", "vs_unpooled_alone"):
                v = entry[key]
                print("  %s is %+.2f us per step against %s (spread %.2f us): %s" % (
                    v["a"], -v["b_minus_a_us"], v["b"], v["spread_us"],
                    "faster by more than the spread" if v["faster_by_more_than_spread"] else
                    "SLOWER by more than the spread" if v["slower_by_more_than_spread"] else "within the spread"))
            sys.stdout.flush()
            del drivers, emb
    finally:
        ops.set_tolerance_mode(prev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
