#!/usr/bin/env python3
"""The HET cache tier of BASELINE configs[1] under the asp-with-prefetch schedule with SUM-POOLED access (the reference's
emb_sum_* models at `--bsp -1`: one embedding_push_pull per training step, a sample's 26 rows summed before the tower),
development aid.  Protocol of tools/cache_pushpull_bench.py and tools/cache_bag_bench.py: LRU, limit = 0.1 x rows, the cache is
filled to its limit first (planned pairs), Criteo batches, chains in blocks of 16 steps with the bookkeeping of the next block
on the side stream.  Per shape (B x F x d), in ONE process, the variants alternating over `--reps` windows; a window is one
whole chain -- head, `--warm` blocks, `--blocks` timed blocks between two device synchronises (host clock), closing entry:
  (a)  the pooled chain step            plan_block(push_pull=True) + run_planned_push_pulls_bags: the push half reads the pooled
                                        gradient [B, d] in place, the pull half sums the rows as it reads them into [B, d];
  (a') the same step through the per-call method embedding_push_pull_planned_bags (the enqueue path of (c));
  (b)  the unpooled chain step alone    run_planned_push_pulls on per-occurrence rows and gradients [n, d] (what
                                        tools/cache_pushpull_bench.py times as "planned push-pull step");
  (c)  what a pooled model pays without (a): IndexedSlices.expanded_values() of the pooled gradient, embedding_push_pull_planned
                                        on [n, d], ops.embedding_lookup_sum over the rows (ids 0 .. n-1).
Reported: median [min .. max] of the windows in us per step, (a) - (c) and (a) - (b) with the larger of the two variants' own
window spreads (a difference inside it counts as none), the algorithmic bytes of (a) and (c) that differ, and one RESULT line.
A planned batch holds at most 36,864 ids: a shape beyond that is reported as not plannable and skipped.
Kernel times: run the tool under rocprofv3 --kernel-trace --stats (the program after `--`)."""
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
from herald_amd import cache as hcache, ops, synth

GS = 16                 # steps per planned block
PLAN_MAX = 36864        # ids of a planned batch (ha_cache_plan_block_push_pull)
SECTION_16_US = 22.16   # docs/EXPERIMENTS.md section 16: tools/cache_pushpull_bench.py's planned push-pull step, 256 x 26 x 512


def bench_shape(dev, rows, B, F, d, reps, nwarm, ntimed, table):
    n = B * F
    versions = torch.zeros(rows, dtype=torch.int64, device=dev)
    hcache.register_table(0, table, versions)
    limit = int(0.1 * rows)
    c = hcache.CacheSparseTable(limit, rows, d, 0, "LRU", bound=100, max_batch=n, device=dev)
    NB = 64
    ids = [torch.from_numpy(np.minimum(synth.as_f32_ids(synth.criteo_batch(B, b, rows=rows, nfields=F)).reshape(-1),
                                       rows - 1)).to(dev) for b in range(NB)]
    rows_buf = torch.empty((n, d), device=dev)                     # per-occurrence rows / gradients
    grad_rows = torch.randn((n, d), device=dev) * 1e-3
    out = torch.empty((B, d), device=dev)                          # pooled rows / gradients
    grad_bags = torch.randn((B, d), device=dev) * 1e-3
    pos = torch.arange(n, dtype=torch.int64, device=dev).reshape(B, F)
    main_s = torch.cuda.Stream(device=dev)
    c.cache.stream = main_s
    c.cache._planned_waits = False
    base = torch.arange(n, device=dev)
    fill = [((base + lo) % rows).to(torch.float32) for lo in range(0, limit + n, n)]
    t0 = time.perf_counter()
    with torch.cuda.stream(main_s):
        blocks = [fill[i:i + GS] for i in range(0, len(fill), GS)]
        c.plan_block(blocks[0])
        for b, blk in enumerate(blocks):
            if b + 1 < len(blocks):
                c.plan_block(blocks[b + 1])
            c.run_planned_pairs([rows_buf] * len(blk), [grad_rows] * len(blk))
    torch.cuda.synchronize()
    print("  fill: %d pairs in %.2f s, size %d / %d" % (len(fill), time.perf_counter() - t0, c.cache.size(), limit))
    blk = [list(range(g0, g0 + GS)) for g0 in range(0, NB, GS)]

    def block(kind, sel_prev):
        if kind == "a":
            c.run_planned_push_pulls_bags([out] * GS, [grad_bags] * GS, F)
        elif kind == "a'":
            for _ in range(GS):
                c.embedding_push_pull_planned_bags(out, grad_bags, bag=F)
        elif kind == "b":
            c.run_planned_push_pulls([rows_buf] * GS, [grad_rows] * GS)
        else:
            for j in sel_prev:              # j: the batch pulled by the step before, whose pooled gradient is pushed now
                g = ops.IndexedSlices(indices=ids[j].reshape(B, F), values=grad_bags, dense_shape=(rows, d), bag=F)
                c.embedding_push_pull_planned(rows_buf, g.expanded_values(stream=main_s))
                ops.embedding_lookup_sum(rows_buf, pos, out=out, stream=main_s)

    def window(kind):
        """One whole chain: head, nwarm + ntimed blocks of GS steps, closing entry; -> us per timed step."""
        pooled = kind in ("a", "a'")

        def plan(b):
            c.plan_block([ids[j] for j in blk[b % len(blk)]], push_pull=True)

        def prev_of(b):                     # the batches pushed by block b's steps
            sel = blk[b % len(blk)]
            first = NB - 1 if b == 0 else blk[(b - 1) % len(blk)][-1]
            return [first] + sel[:-1]

        with torch.cuda.stream(main_s):
            c.plan_block([ids[NB - 1]], push_pull=True)          # the chain's head
            plan(0)
            if pooled:
                c.embedding_push_pull_planned_bags(out, None, bag=F)
            else:
                c.embedding_lookup_planned(rows_buf)
            for b in range(nwarm + ntimed):
                if b == nwarm:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if b + 1 < nwarm + ntimed:
                    plan(b + 1)
                block(kind, prev_of(b))
            torch.cuda.synchronize()
            t = 1e6 * (time.perf_counter() - t0) / (ntimed * GS)
            c.plan_block([None], push_pull=True)                 # the closing entry
            if pooled:
                c.embedding_push_pull_planned_bags(None, grad_bags, bag=F)
            else:
                c.embedding_update_planned(grad_rows)
            torch.cuda.synchronize()
            return t

    kinds = ("a", "b", "c", "a'")
    got = {k: [] for k in kinds}
    for k in kinds:                          # every variant warmed once: code objects, allocator, workspaces
        window(k)
    for _ in range(reps):
        for k in kinds:
            got[k].append(window(k))
    del c
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x512,4096x26x128,1024x26x128", help="B x F x d, comma separated")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=7, help="timed windows (whole chains) per variant")
    ap.add_argument("--warm", type=int, default=2, help="untimed blocks at the start of every window")
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks of 16 steps per window")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cache_bag_pushpull_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    names = {"a": "pooled chain step (native loop)", "a'": "pooled chain step (per-call)", "b": "unpooled chain step alone",
             "c": "unpooled step + sum pass + expansion"}
    results = {"rows": args.rows, "reps": args.reps, "blocks": args.blocks, "device": torch.cuda.get_device_name(dev),
               "shapes": {}}
    table, table_d = None, None
    for B, F, d in [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]:
        n, tag = B * F, "%dx%dx%d" % (B, F, d)
        print("== B=%d F=%d d=%d  n=%d" % (B, F, d, n))
        if n > PLAN_MAX:
            print("  not plannable: a planned batch holds at most %d ids (plan_block refuses %d); skipped" % (PLAN_MAX, n))
            results["shapes"][tag] = {"n": n, "skipped": "n > %d" % PLAN_MAX}
            continue
        if table_d != d:
            table = None
            torch.cuda.empty_cache()
            table, table_d = init_table(args.rows, d, dev), d
        got = bench_shape(dev, args.rows, B, F, d, args.reps, args.warm, args.blocks, table)
        res = {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v)), "windows": len(v),
                   "windows_us": [round(float(x), 2) for x in v]} for k, v in got.items()}
        for k in ("a", "a'", "b", "c"):
            r = res[k]
            print("  (%-2s) %-38s median %7.2f us per step  [%7.2f .. %7.2f]  %d windows of %d steps" % (
                k, names[k], r["median_us"], r["min_us"], r["max_us"], r["windows"], args.blocks * GS))
        cmp_ = {}
        for x, y in (("a", "c"), ("a", "b"), ("a'", "c")):
            spread = max(res[x]["max_us"] - res[x]["min_us"], res[y]["max_us"] - res[y]["min_us"])
            diff = res[x]["median_us"] - res[y]["median_us"]
            cmp_["%s-%s" % (x, y)] = {"diff_us": diff, "spread_us": spread, "inside_spread": bool(abs(diff) <= spread)}
            print("  (%s) - (%s): %+.2f us, spread %.2f us%s" % (x, y, diff, spread,
                                                               "  -- inside the spread" if abs(diff) <= spread else ""))
        d4 = 4 * d
        # bytes per step that differ between (a) and (c): the traffic of lines, store rows and versions is the same
        pooled_b = {"pull": n * d4 + B * d4, "sum_pass": 0, "push_side": B * d4}
        unpooled_b = {"pull": n * (2 * d4 + 4), "sum_pass": n * (d4 + 8) + B * d4, "push_side": (B * d4 + n * d4) + n * d4}
        print("  algorithmic bytes per step, (a): %d   (c): %d" % (sum(pooled_b.values()), sum(unpooled_b.values())))
        if (B, F, d) == (256, 26, 512):
            print("  sanity: (b) is the protocol of tools/cache_pushpull_bench.py's planned push-pull step, %.2f us in "
                  "docs/EXPERIMENTS.md section 16; here %.2f" % (SECTION_16_US, res["b"]["median_us"]))
        results["shapes"][tag] = {"n": n, "variants": res, "differences": cmp_, "bytes_a": sum(pooled_b.values()),
                                  "bytes_c": sum(unpooled_b.values())}
        print("RESULT shape=%s a_us=%.2f a_call_us=%.2f b_us=%.2f c_us=%.2f a_minus_c_us=%+.2f a_minus_b_us=%+.2f" % (
            tag, res["a"]["median_us"], res["a'"]["median_us"], res["b"]["median_us"], res["c"]["median_us"],
            cmp_["a-c"]["diff_us"], cmp_["a-b"]["diff_us"]))
        sys.stdout.flush()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
