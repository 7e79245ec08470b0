#!/usr/bin/env python3
"""The HET cache tier of BASELINE configs[1] with PUSH KEYS (the update of the laia scheduler's push plans,
cache.cc:248-335), development aid: limit = 0.1 x rows, wdl_criteo bs=256 d=512 batches, every batch pushing a sorted random
third of its unique keys.  The cache is filled to its limit first (planned pairs), then, in this order and timed once each
(first-try numbers, no best-of):
  planned push-key pairs   blocks of 16 pairs: plan_block(..., push_keys_list=...) + run_planned_pairs (ONE launch per
                           lookup and per update; bookkeeping + push-key marks on the side stream);
  planned bound pairs      the same blocks without push keys (the plain planned pair, for comparison);
  call-by-call pairs       embedding_lookup + embedding_update_with_push_keys.
POLICY (LRU / LFU / LFUOpt) / ROWS / WIDTH / BLOCKS.  Under rocprofv3 --kernel-trace --stats the kernel times of the mark
(cache_plan_push_mark_kernel) and bookkeeping (cache_book_block_kernel / cache_book_lfu_kernel) launches come from its stats."""
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
    policy = os.environ.get("POLICY", "LRU")
    n = bs * 26
    table = torch.empty((rows, width), device=dev)
    for s in range(0, rows, 1 << 20):
        table[s:s + (1 << 20)].normal_(0, 0.01)
    versions = torch.zeros(rows, dtype=torch.int64, device=dev)
    hcache.register_table(0, table, versions)
    limit = int(0.1 * rows)
    c = hcache.CacheSparseTable(limit, rows, width, 0, policy, bound=100, max_batch=n, device=dev)
    rng = np.random.default_rng(0)
    NB = 256
    ids_h = [np.minimum(synth.as_f32_ids(synth.criteo_batch(bs, b, rows=rows)).reshape(-1), rows - 1) for b in range(NB)]
    ids = [torch.from_numpy(x).to(dev) for x in ids_h]
    pks = []
    for x in ids_h:
        u = np.unique(x)
        pks.append(torch.from_numpy(np.sort(rng.choice(u, size=u.size // 3, replace=False))).to(dev))
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

    def planned(with_pk):
        blk = [list(range(g0, g0 + GS)) for g0 in range(0, NB, GS)]

        def plan(b):
            sel = blk[b % len(blk)]
            c.plan_block([ids[j] for j in sel], push_keys_list=[pks[j] for j in sel] if with_pk else None)

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

    t_pk = planned(True)
    print("planned push-key pair: %.2f us (%d pairs, first try)" % (t_pk, ntimed * GS))
    t_bound = planned(False)
    print("planned bound pair:    %.2f us (%d pairs, first try)" % (t_bound, ntimed * GS))
    with torch.cuda.stream(main_s):
        for k in range(32):
            c.embedding_lookup(ids[k], out)
            c.embedding_update_with_push_keys(ids[k], pks[k], grad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        npairs = ntimed * GS
        for k in range(32, 32 + npairs):
            c.embedding_lookup(ids[k % NB], out)
            c.embedding_update_with_push_keys(ids[k % NB], pks[k % NB], grad)
        torch.cuda.synchronize()
        t_cbc = 1e6 * (time.perf_counter() - t0) / npairs
    print("call-by-call push-key pair: %.2f us (%d pairs, first try)" % (t_cbc, npairs))
    print("RESULT policy=%s planned_pushkeys_us=%.2f planned_bound_us=%.2f call_by_call_pushkeys_us=%.2f" % (
        policy, t_pk, t_bound, t_cbc))


if __name__ == "__main__":
    main()
