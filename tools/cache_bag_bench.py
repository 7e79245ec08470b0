#!/usr/bin/env python3
"""The HET cache tier of BASELINE configs[1] under SUM-POOLED access (the reference's emb_sum_* models: a sample's 26 rows are
summed before the tower), development aid: limit = 0.1 x rows, wdl_criteo bs=256 d=512 batches in blocks of 16.  The cache is
filled to its limit first (planned pairs), then each of the following is timed once per round, the rounds alternating twice so
the spread between repeats is visible (first-try numbers, no best-of):
  (a)  fused pooled pairs    plan_block + run_planned_pairs_bags: ONE launch per lookup (rows summed as they are read, out is
                             [B, d]) and ONE per update (the pooled gradient [B, d] read in place);
  (a') the same pairs through the per-call methods embedding_lookup_sum_planned / embedding_update_planned_bags (the enqueue
       path of (b): one Python call per launch);
  (b)  unfused pooled pairs  embedding_lookup_planned into [n, d] rows, ops.embedding_lookup_sum over them (ids 0 .. n-1),
                             IndexedSlices.expanded_values() of the pooled gradient, embedding_update_planned on [n, d];
  (c)  the plain pair        run_planned_pairs on per-occurrence rows and gradients (no pooling at all).
POLICY (LRU / LFU / LFUOpt) / ROWS / WIDTH / BLOCKS from the environment.  Kernel times: run the tool under
rocprofv3 --kernel-trace --stats (the program after `--`)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from herald_amd import cache as hcache, ops, synth


def main():
    if not torch.cuda.is_available():
        sys.exit("cache_bag_bench: no GPU found")
    dev = torch.device("cuda:0")
    rows = int(os.environ.get("ROWS", "33762577"))
    width, bs, F = int(os.environ.get("WIDTH", "512")), 256, 26
    policy = os.environ.get("POLICY", "LRU")
    n = bs * F
    table = torch.empty((rows, width), device=dev)
    for s in range(0, rows, 1 << 20):
        table[s:s + (1 << 20)].normal_(0, 0.01)
    versions = torch.zeros(rows, dtype=torch.int64, device=dev)
    hcache.register_table(0, table, versions)
    limit = int(0.1 * rows)
    c = hcache.CacheSparseTable(limit, rows, width, 0, policy, bound=100, max_batch=n, device=dev)
    NB = 256
    ids_h = [np.minimum(synth.as_f32_ids(synth.criteo_batch(bs, b, rows=rows)).reshape(-1), rows - 1) for b in range(NB)]
    ids = [torch.from_numpy(x).to(dev) for x in ids_h]
    rows_buf = torch.empty((n, width), device=dev)                 # per-occurrence rows / gradients
    grad_rows = torch.randn((n, width), device=dev) * 1e-3
    out = torch.empty((bs, width), device=dev)                     # pooled rows / gradients
    grad_bags = torch.randn((bs, width), device=dev) * 1e-3
    pos = torch.arange(n, dtype=torch.int64, device=dev).reshape(bs, F)
    main_s = torch.cuda.Stream(device=dev)
    c.cache.stream = main_s
    c.cache._planned_waits = False
    GS = 16
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
    print("fill: %d pairs in %.2f s, size %d / %d, policy %s" % (len(fill), time.perf_counter() - t0, c.cache.size(), limit,
                                                                policy))
    nwarm, ntimed = 4, int(os.environ.get("BLOCKS", "16"))
    blk = [list(range(g0, g0 + GS)) for g0 in range(0, NB, GS)]

    def block_fused_native():
        c.run_planned_pairs_bags([out] * GS, [grad_bags] * GS, F)

    def block_fused_calls():
        for _ in range(GS):
            c.embedding_lookup_sum_planned(out, bag=F)
            c.embedding_update_planned_bags(grad_bags, bag=F)

    def block_unfused(sel):
        for j in sel:
            c.embedding_lookup_planned(rows_buf)
            ops.embedding_lookup_sum(rows_buf, pos, out=out, stream=main_s)
            g = ops.IndexedSlices(indices=ids[j].reshape(bs, F), values=grad_bags, dense_shape=(rows, width), bag=F)
            c.embedding_update_planned(g.expanded_values(stream=main_s))

    def block_plain():
        c.run_planned_pairs([rows_buf] * GS, [grad_rows] * GS)

    def timed(kind):
        with torch.cuda.stream(main_s):
            c.plan_block([ids[j] for j in blk[0]])
            for b in range(nwarm + ntimed):
                if b == nwarm:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if b + 1 < nwarm + ntimed:
                    c.plan_block([ids[j] for j in blk[(b + 1) % len(blk)]])
                if kind == "a":
                    block_fused_native()
                elif kind == "a'":
                    block_fused_calls()
                elif kind == "b":
                    block_unfused(blk[b % len(blk)])
                else:
                    block_plain()
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0) / (ntimed * GS)

    names = {"a": "fused pooled pair (native loop)", "a'": "fused pooled pair (per-call)", "b": "unfused pooled pair",
             "c": "plain per-occurrence pair"}
    got = {k: [] for k in names}
    for rnd in range(2):
        for k in ("a", "b", "c", "a'"):
            got[k].append(timed(k))
            print("round %d  (%s) %-34s %.2f us per pair (%d pairs)" % (rnd, k, names[k], got[k][-1], ntimed * GS))
    # algorithmic bytes per pair that differ between (a) and (b) -- the traffic of lines, store rows and versions is the same
    d4 = 4 * width
    fused = {"lookup": n * d4 + bs * d4, "sum_pass": 0, "update_side": bs * d4}
    unfused = {"lookup": n * (2 * d4 + 4), "sum_pass": n * (d4 + 8) + bs * d4,
               "update_side": (bs * d4 + n * d4) + n * d4}      # expand (read [B, d], write [n, d]) + gradient reads
    print("algorithmic bytes per pair, fused:   lookup %d  sum pass %d  update side %d  total %d" % (
        fused["lookup"], fused["sum_pass"], fused["update_side"], sum(fused.values())))
    print("algorithmic bytes per pair, unfused: lookup %d  sum pass %d  update side %d  total %d" % (
        unfused["lookup"], unfused["sum_pass"], unfused["update_side"], sum(unfused.values())))
    print("RESULT policy=%s fused_us=%.2f,%.2f fused_per_call_us=%.2f,%.2f unfused_us=%.2f,%.2f plain_us=%.2f,%.2f "
          "fused_bytes=%d unfused_bytes=%d fused_faster_first_try=%s" % (
              policy, got["a"][0], got["a"][1], got["a'"][0], got["a'"][1], got["b"][0], got["b"][1], got["c"][0], got["c"][1],
              sum(fused.values()), sum(unfused.values()), got["a"][0] < got["b"][0]))


if __name__ == "__main__":
    main()
