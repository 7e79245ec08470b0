#!/usr/bin/env python3
"""The HET cache tier of BASELINE configs[1] under SUM-POOLED access through the cache's CALL-BY-CALL interface (the callers the
planned flow does not reach: a remote store, LFU / LFUOpt on the asp schedule, no ids a block ahead), development aid: limit =
0.1 x rows, the cache filled to its limit first (planned pairs, as tools/cache_bag_bench.py), criteo batches of BATCH x 26 ids.
For every policy of POLICIES, a lookup + update pair and a push-pull step are timed in three legs, in the same process:
  pooled     embedding_lookup_sum + embedding_update_bags(same_as_lookup=True)   /   embedding_push_pull_bags
  unpooled   embedding_lookup + embedding_update(same_as_lookup=True)            /   embedding_push_pull      (no pooling at all)
  yardstick  what a pooled model pays without the pooled calls: the unpooled calls + ops.embedding_lookup_sum over the
             delivered [n, d] rows (ids 0 .. n-1) + IndexedSlices.expanded_values() of the pooled gradient
Reported: us per step, median [min .. max] of 7 windows of STEPS steps, the legs taking turns window by window; first try, no
best-of.  ROWS / WIDTH / BATCH / STEPS / POLICIES (default LRU,LFU) from the environment.  Kernel times: run the tool under
rocprofv3 --kernel-trace --stats (the program after `--`)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from herald_amd import cache as hcache, ops, synth

F, WINDOWS = 26, 7


def main():
    if not torch.cuda.is_available():
        sys.exit("cache_bag_calls_bench: no GPU found")
    dev = torch.device("cuda:0")
    rows = int(os.environ.get("ROWS", "33762577"))
    width, bs = int(os.environ.get("WIDTH", "512")), int(os.environ.get("BATCH", "256"))
    steps = int(os.environ.get("STEPS", "64"))
    policies = os.environ.get("POLICIES", "LRU,LFU").split(",")
    n = bs * F
    table = torch.empty((rows, width), device=dev)
    for s in range(0, rows, 1 << 20):
        table[s:s + (1 << 20)].normal_(0, 0.01)
    limit = int(0.1 * rows)
    NB = 64
    ids = [torch.from_numpy(np.minimum(synth.as_f32_ids(synth.criteo_batch(bs, b, rows=rows)).reshape(-1), rows - 1)).to(dev)
           for b in range(NB)]
    rows_buf = torch.empty((n, width), device=dev)                 # per-occurrence rows / gradients
    grad_rows = torch.randn((n, width), device=dev) * 1e-3
    out = torch.empty((bs, width), device=dev)                     # pooled rows / gradients
    grad_bags = torch.randn((bs, width), device=dev) * 1e-3
    pos = torch.arange(n, dtype=torch.int64, device=dev).reshape(bs, F)
    main_s = torch.cuda.Stream(device=dev)
    print("shape %d x %d x %d, rows %d, limit %d, %d windows of %d steps" % (bs, F, width, rows, limit, WINDOWS, steps))
    for policy in policies:
        versions = torch.zeros(rows, dtype=torch.int64, device=dev)
        hcache.register_table(0, table, versions)
        c = hcache.CacheSparseTable(limit, rows, width, 0, policy, bound=100, max_batch=n, device=dev)
        c.cache.stream = main_s
        c.cache._planned_waits = False
        base = torch.arange(n, device=dev)
        fill = [((base + lo) % rows).to(torch.float32) for lo in range(0, limit + n, n)]
        t0 = time.perf_counter()
        with torch.cuda.stream(main_s):
            blocks = [fill[i:i + 16] for i in range(0, len(fill), 16)]
            c.plan_block(blocks[0])
            for b, blk in enumerate(blocks):
                if b + 1 < len(blocks):
                    c.plan_block(blocks[b + 1])
                c.run_planned_pairs([rows_buf] * len(blk), [grad_rows] * len(blk))
        torch.cuda.synchronize()
        print("fill: %d pairs in %.2f s, size %d / %d, policy %s" % (len(fill), time.perf_counter() - t0, c.cache.size(), limit,
                                                                    policy), flush=True)
        del fill, blocks

        def expanded(j):
            g = ops.IndexedSlices(indices=ids[j].reshape(bs, F), values=grad_bags, dense_shape=(rows, width), bag=F)
            return g.expanded_values(stream=main_s)

        def pair(leg, j):
            if leg == "pooled":
                c.embedding_lookup_sum(ids[j], out, bag=F)
                c.embedding_update_bags(ids[j], grad_bags, bag=F, same_as_lookup=True)
            elif leg == "unpooled":
                c.embedding_lookup(ids[j], rows_buf)
                c.embedding_update(ids[j], grad_rows, same_as_lookup=True)
            else:
                c.embedding_lookup(ids[j], rows_buf)
                ops.embedding_lookup_sum(rows_buf, pos, out=out, stream=main_s)
                c.embedding_update(ids[j], expanded(j), same_as_lookup=True)

        def push_pull(leg, j):
            nxt = (j + 1) % NB
            if leg == "pooled":
                c.embedding_push_pull_bags(ids[nxt], out, ids[j], grad_bags, bag=F)
            elif leg == "unpooled":
                c.embedding_push_pull(ids[nxt], rows_buf, ids[j], grad_rows)
            else:
                c.embedding_push_pull(ids[nxt], rows_buf, ids[j], expanded(j))
                ops.embedding_lookup_sum(rows_buf, pos, out=out, stream=main_s)

        legs = ("pooled", "unpooled", "yardstick")
        for what, step_fn in (("lookup + update pair", pair), ("push-pull step", push_pull)):
            got = {leg: [] for leg in legs}
            k = 0
            with torch.cuda.stream(main_s):
                for leg in legs:                                   # warm-up: every leg's kernels loaded, the cache in the schedule
                    for _ in range(8):
                        step_fn(leg, k % NB)
                        k += 1
                for _ in range(WINDOWS):
                    for leg in legs:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(steps):
                            step_fn(leg, k % NB)
                            k += 1
                        torch.cuda.synchronize()
                        got[leg].append(1e6 * (time.perf_counter() - t0) / steps)
            for leg in legs:
                v = sorted(got[leg])
                print("RESULT policy=%s shape=%dx%dx%d %-22s %-9s %8.1f us per step  [%.1f .. %.1f]" % (
                    policy, bs, F, width, what, leg, v[len(v) // 2], v[0], v[-1]), flush=True)
            po, ya = sorted(got["pooled"]), sorted(got["yardstick"])
            print("RESULT policy=%s shape=%dx%dx%d %-22s pooled_faster_outside_the_spread=%s" % (
                policy, bs, F, width, what, po[-1] < ya[0]), flush=True)
        del c
        hcache._TABLES.pop(0, None)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
