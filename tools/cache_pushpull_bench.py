#!/usr/bin/env python3
"""The HET cache tier of BASELINE configs[1] under the asp-with-prefetch schedule (one embedding_push_pull per training step,
cache.cc:356-422), development aid: limit = 0.1 x rows, wdl_criteo bs=256 d=512 batches.  The cache is filled to its limit
first (planned pairs), then, in one process, in this order and timed once each (first-try numbers, no best-of):
  planned push-pull steps  a chain in blocks of 16 steps: plan_block(..., push_pull=True) + run_planned_push_pulls (two row
                           launches per step, the bookkeeping of the next block on the side stream); the chain is closed;
  planned bound pairs      blocks of 16 lookup + update pairs of the same batches (the same rows in two launches);
  call-by-call steps       embedding_push_pull(pull = batch k + 1, push = batch k).
ROWS / WIDTH / BLOCKS.  Under rocprofv3 --kernel-trace --stats the kernel times of the bookkeeping launch
(cache_book_chain_kernel, one per block) and of the row launches (cache_update_planned_kernel, cache_lookup_planned_kernel)
come from its stats."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from herald_amd import cache as hcache, synth


def main():
    dev = torch.device("cuda:0")
    rows = int(os.environ.get("ROWS", "33762577"))
    width, bs = int(os.environ.get("WIDTH", "512")), 256
    policy = "LRU"
    n = bs * 26
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
    out = torch.empty((n, width), device=dev)
    grad = torch.randn((n, width), device=dev) * 1e-3
    main_s = torch.cuda.Stream(device=dev)
    c.cache.stream = main_s
    GS = 16
    outs, grads = [out] * GS, [grad] * GS
    base = torch.arange(n, device=dev)
    fill = [((base + lo) % rows).to(torch.float32) for lo in range(0, limit + n, n)]
    t0 = time.perf_counter()
    with torch.cuda.stream(main_s):
        blocks = [fill[i:i + GS] for i in range(0, len(fill), GS)]
        c.plan_block(blocks[0])
        for b, blk in enumerate(blocks):
            if b + 1 < len(blocks):
                c.plan_block(blocks[b + 1])
            c.run_planned_pairs(outs[:len(blk)], grads[:len(blk)])
    torch.cuda.synchronize()
    print("fill: %d pairs in %.2f s, size %d / %d, policy %s" % (len(fill), time.perf_counter() - t0, c.cache.size(), limit,
                                                                policy))
    nwarm, ntimed = 4, int(os.environ.get("BLOCKS", "16"))
    blk = [list(range(g0, g0 + GS)) for g0 in range(0, NB, GS)]

    def chain():
        def plan(b):
            c.plan_block([ids[j] for j in blk[b % len(blk)]], push_pull=True)

        with torch.cuda.stream(main_s):
            c.plan_block([ids[NB - 1]], push_pull=True)      # the chain's head
            plan(0)
            c.embedding_lookup_planned(out)
            for b in range(nwarm + ntimed):
                if b == nwarm:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if b + 1 < nwarm + ntimed:
                    plan(b + 1)
                c.run_planned_push_pulls(outs, grads)
            torch.cuda.synchronize()
            t = 1e6 * (time.perf_counter() - t0) / (ntimed * GS)
            c.plan_block([None], push_pull=True)             # the closing step
            c.embedding_update_planned(grad)
            torch.cuda.synchronize()
            return t

    def pairs():
        def plan(b):
            c.plan_block([ids[j] for j in blk[b % len(blk)]])

        with torch.cuda.stream(main_s):
            plan(0)
            for b in range(nwarm + ntimed):
                if b == nwarm:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if b + 1 < nwarm + ntimed:
                    plan(b + 1)
                c.run_planned_pairs(outs, grads)
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0) / (ntimed * GS)

    t_pp = chain()
    print("planned push-pull step: %.2f us (%d steps, first try)" % (t_pp, ntimed * GS))
    t_pair = pairs()
    print("planned bound pair:     %.2f us (%d pairs, first try)" % (t_pair, ntimed * GS))
    with torch.cuda.stream(main_s):
        c.embedding_lookup(ids[NB - 1], out)
        for k in range(32):
            c.embedding_push_pull(ids[k], out, ids[(k - 1) % NB], grad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nsteps = ntimed * GS
        for k in range(32, 32 + nsteps):
            c.embedding_push_pull(ids[k % NB], out, ids[(k - 1) % NB], grad)
        torch.cuda.synchronize()
        t_cbc = 1e6 * (time.perf_counter() - t0) / nsteps
        c.embedding_update(ids[(31 + nsteps) % NB], grad)
        torch.cuda.synchronize()
    print("call-by-call push-pull step: %.2f us (%d steps, first try)" % (t_cbc, nsteps))
    print("RESULT policy=LRU planned_push_pull_us=%.2f planned_bound_pair_us=%.2f call_by_call_push_pull_us=%.2f" % (
        t_pp, t_pair, t_cbc))


if __name__ == "__main__":
    main()
