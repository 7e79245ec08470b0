#!/usr/bin/env python3
"""The HET cache tier of BASELINE configs[1] under WEIGHTED sum-pooled access (the reference's FAE models: a sample's 26 rows
are multiplied by the 0/1 mask of the cold ids and summed), development aid; tools/cache_bag_bench.py's protocol: limit = 0.1 x
rows, filled first, wdl_criteo bs=256 batches in blocks of 16, everything in one process, each of the following timed once per
round, two rounds (first-try numbers, no best-of), for synthetic dead shares of 0 / 50 / 85 % with the dead slots on id 0:
  (a)  fused weighted pairs   plan_block + run_planned_pairs_wbags: ONE launch per lookup (rows multiplied and summed as they are
                              read) and ONE per update (the pooled gradient [B, d] and the weights read in place, dead
                              occurrences skipped);
  (a') the same pairs through the per-call methods embedding_lookup_wsum_planned / embedding_update_planned_wbags;
  (b)  composed pairs         embedding_lookup_planned into [n, d] rows, ops.embedding_lookup_wsum over them, ops.wbag_grad_rows
                              into [n, d], the scale, embedding_update_planned on [n, d];
  (c)  the unweighted sum-pooled pair, run_planned_pairs_bags, on the same ids: what the weights cost.
POLICY (LRU / LFU / LFUOpt) / ROWS / WIDTH / BLOCKS / SHARES from the environment.  Kernel times: run the tool under
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
        sys.exit("cache_wbag_bench: no GPU found")
    dev = torch.device("cuda:0")
    rows = int(os.environ.get("ROWS", "33762577"))
    width, bs, F = int(os.environ.get("WIDTH", "512")), 256, 26
    policy = os.environ.get("POLICY", "LRU")
    shares = [float(x) for x in os.environ.get("SHARES", "0,0.5,0.85").split(",")]
    scale = -0.01
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
    print("fill: %d pairs in %.2f s, size %d / %d, policy %s, width %d" % (len(fill), time.perf_counter() - t0, c.cache.size(),
                                                                           limit, policy, width))
    nwarm, ntimed = 4, int(os.environ.get("BLOCKS", "16"))
    blk = [list(range(g0, g0 + GS)) for g0 in range(0, NB, GS)]
    names = {"a": "fused weighted pair (native loop)", "a'": "fused weighted pair (per-call)", "b": "composed weighted pair",
             "c": "unweighted sum-pooled pair"}
    d4 = 4 * width
    fused = {"lookup": n * (d4 + 4) + bs * d4, "sum_pass": 0, "update_side": bs * d4 + n * 4}
    composed = {"lookup": n * (2 * d4 + 4), "sum_pass": n * (d4 + 8 + 4) + bs * d4,
                # wbag_grad_rows (read [B, d] and the weights, write [n, d]) + the scale (read, write) + gradient reads
                "update_side": (bs * d4 + n * 4 + n * d4) + 2 * n * d4 + n * d4}
    print("algorithmic bytes per pair that differ, fused:    lookup %d  sum pass %d  update side %d  total %d" % (
        fused["lookup"], fused["sum_pass"], fused["update_side"], sum(fused.values())))
    print("algorithmic bytes per pair that differ, composed: lookup %d  sum pass %d  update side %d  total %d" % (
        composed["lookup"], composed["sum_pass"], composed["update_side"], sum(composed.values())))
    rng = np.random.default_rng(5)
    results = []
    for share in shares:
        ids, ws = [], []
        for x in ids_h:
            dead = rng.random(n) < share
            y = x.copy()
            y[dead] = 0
            ids.append(torch.from_numpy(y).to(dev))
            ws.append(torch.from_numpy((~dead).astype(np.float32)).to(dev).reshape(bs, F))

        def timed(kind):
            with torch.cuda.stream(main_s):
                c.plan_block([ids[j] for j in blk[0]])
                for b in range(nwarm + ntimed):
                    if b == nwarm:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    if b + 1 < nwarm + ntimed:
                        c.plan_block([ids[j] for j in blk[(b + 1) % len(blk)]])
                    sel = blk[b % len(blk)]
                    if kind == "a":
                        c.run_planned_pairs_wbags([out] * GS, [grad_bags] * GS, [ws[j] for j in sel], F, scale=scale)
                    elif kind == "a'":
                        for j in sel:
                            c.embedding_lookup_wsum_planned(out, ws[j], bag=F)
                            c.embedding_update_planned_wbags(grad_bags, ws[j], bag=F, scale=scale)
                    elif kind == "b":
                        for j in sel:
                            c.embedding_lookup_planned(rows_buf)
                            ops.embedding_lookup_wsum(rows_buf, pos, ws[j], out=out, stream=main_s)
                            ops.wbag_grad_rows(grad_bags, ws[j], bag=F, out=grad_rows, stream=main_s)
                            grad_rows.mul_(scale)
                            c.embedding_update_planned(grad_rows)
                    else:
                        c.run_planned_pairs_bags([out] * GS, [grad_bags] * GS, F)
                torch.cuda.synchronize()
                return 1e6 * (time.perf_counter() - t0) / (ntimed * GS)

        got = {k: [] for k in names}
        for rnd in range(2):
            for k in ("a", "b", "c", "a'"):
                got[k].append(timed(k))
                print("dead %.2f round %d  (%s) %-34s %.2f us per pair (%d pairs)" % (share, rnd, k, names[k], got[k][-1],
                                                                                     ntimed * GS))
        results.append("dead=%.2f fused_us=%.2f,%.2f fused_per_call_us=%.2f,%.2f composed_us=%.2f,%.2f sum_pooled_us=%.2f,%.2f" % (
            share, got["a"][0], got["a"][1], got["a'"][0], got["a'"][1], got["b"][0], got["b"][1], got["c"][0], got["c"][1]))
    print("RESULT policy=%s width=%d fused_bytes=%d composed_bytes=%d | %s" % (policy, width, sum(fused.values()),
                                                                              sum(composed.values()), " | ".join(results)))


if __name__ == "__main__":
    main()
