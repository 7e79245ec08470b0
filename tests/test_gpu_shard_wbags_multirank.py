"""ShardedEmbedding.pull_wsum / push_wbags / push_pull_wbags with the HIP engine at world sizes 2 and 4 on ONE GPU, in the
manner of tests/test_gpu_shard_bags_multirank.py: every rank is a process with its own shard on cuda:0, the collectives run on a
gloo group and the buffers are staged through the host for them (the store's `a2a` hook).  Weighted pooled rows against
tests/wbag_model.py on the global table (the twin's shards, gathered), tables and stats against a twin store driven through pull /
push of the expanded values (ops.wbag_grad_rows) in the same workers.  Bit patterns throughout."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 26


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def host_staged_a2a(out, inp, out_splits, in_splits, group):
    torch.cuda.current_stream().synchronize()
    o = torch.empty(out.shape, dtype=out.dtype)
    dist.all_to_all_single(o, inp.cpu(), out_splits, in_splits, group=group)
    out.copy_(o)


def _offsets(n, nbags, seed):
    """Ragged bags with empty ones at the front, in the middle and at the end."""
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, nbags - 4))
    h = cuts.size // 2
    return np.concatenate([[0, 0], cuts[:h], [cuts[h]], cuts[h:], [n, n]]).astype(np.int64)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _worker(rank, world, port, rows, width, B, ragged_odd):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    import wbag_model
    from herald_amd import ops
    from herald_amd.sharded import ShardedEmbedding, partition

    n = B * F
    rng = np.random.default_rng(4321)              # the same stream on every rank
    table_g = rng.standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)

    def store():
        return ShardedEmbedding(rows, width, dev, a2a=host_staged_a2a,
                                table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()).to(dev))

    emb, twin = store(), store()
    lr = 0.05

    def batch(step, r):
        """FAE data: half of the slots dead, naming the padding id 0 (the batch's longest run, owned by rank 0)."""
        g = np.random.default_rng(step * 100 + r)
        ids = g.integers(0, rows, size=n).astype(np.float32)
        ids[: n // 4] = np.random.default_rng(step).integers(0, rows, size=n // 4)     # keys shared between ranks
        w = g.standard_normal(n, dtype=np.float32)
        dead = g.random(n) < 0.5
        ids[dead], w[dead] = 0, 0
        ids[1:60:2], w[1:60:2] = ids[1], 0.5                                          # a long run with live occurrences
        return ids, w

    def grads(step, r):
        return np.random.default_rng(7 + step * world + r).standard_normal((B, width), dtype=np.float32)

    def offs(step):
        return _offsets(n, B, step) if ragged_odd and step % 2 else None

    def shaped(a, off):
        t = torch.from_numpy(a).to(dev)
        return t if off is not None else t.view(B, F)

    def table_now():
        parts = [None] * world
        dist.all_gather_object(parts, twin.table.cpu().numpy())
        return np.concatenate(parts)

    def pooled(table, ids, w, off):
        return wbag_model.wbag_sum(table, ids if off is not None else ids.reshape(B, F), w if off is not None else w.reshape(B, F),
                                   off)

    def expanded(g, w, off):
        d_off = torch.from_numpy(off).to(dev) if off is not None else None
        return ops.wbag_grad_rows(torch.from_numpy(g).to(dev), torch.from_numpy(w).to(dev), bag=None if off is not None else F,
                                  bag_of=ops.bag_of(d_off, n) if off is not None else None)

    steps = 3
    route = emb.prefetch(shaped(batch(0, rank)[0], offs(0)), after_current=False)
    for k in range(steps):
        off = offs(k)
        d_off = torch.from_numpy(off).to(dev) if off is not None else None
        cur = route
        if k + 1 < steps:
            route = emb.prefetch(shaped(batch(k + 1, rank)[0], offs(k + 1)), after_current=False)
        ids, w = batch(k, rank)
        torch.cuda.synchronize()
        want = table_now()
        d_w = shaped(w, off)
        got = emb.pull_wsum(weights=d_w, offsets=d_off, route=cur)
        torch.cuda.synchronize()
        assert got.shape == (B, width)
        np.testing.assert_array_equal(_bits(got), _bits(pooled(want, ids, w, off)),
                                      err_msg="pull_wsum, step %d rank %d" % (k, rank))
        assert np.any(_bits(got))
        d_flat = torch.from_numpy(ids).to(dev)
        twin.pull(d_flat)
        g = grads(k, rank)
        d_g = torch.from_numpy(g).to(dev)
        emb.push_wbags(None, d_g, d_w, lr, offsets=d_off, route=cur)
        before = _bits(twin.table).copy()
        twin.push(d_flat, expanded(g, w, off), lr)
        if k + 1 < steps:
            emb.complete(route)
        torch.cuda.synchronize()
        dist.barrier()
        np.testing.assert_array_equal(_bits(d_g), _bits(g))                 # inputs as they were
        np.testing.assert_array_equal(_bits(d_w).reshape(-1), _bits(w))
        np.testing.assert_array_equal(_bits(emb.table), _bits(twin.table),
                                      err_msg="shard after push_wbags, step %d rank %d" % (k, rank))
        assert not np.array_equal(_bits(twin.table), before)
        assert emb.stats == twin.stats

    # push_pull_wbags: every rank's push is applied (rank order) before any rank's pull is served
    off_push, off_pull = offs(9), offs(10)
    (ids_p, w_p), (ids_n, w_n) = batch(9, rank), batch(10, rank)
    g = grads(9, rank)
    got = emb.push_pull_wbags(shaped(ids_p, off_push), torch.from_numpy(g).to(dev), shaped(w_p, off_push), lr,
                              shaped(ids_n, off_pull), shaped(w_n, off_pull),
                              push_offsets=torch.from_numpy(off_push).to(dev) if off_push is not None else None,
                              pull_offsets=torch.from_numpy(off_pull).to(dev) if off_pull is not None else None)
    twin.push_pull(torch.from_numpy(ids_p).to(dev), expanded(g, w_p, off_push), lr, torch.from_numpy(ids_n).to(dev))
    torch.cuda.synchronize()
    dist.barrier()
    want = table_now()
    np.testing.assert_array_equal(_bits(got), _bits(pooled(want, ids_n, w_n, off_pull)), err_msg="push_pull_wbags rows")
    np.testing.assert_array_equal(_bits(emb.table), _bits(twin.table))
    assert emb.stats == twin.stats and emb.stats["xgmi_bytes_out"] > 0
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,rows,width,B,ragged_odd", [(2, 5000, 64, 50, False), (4, 20000, 33, 100, True)])
def test_weighted_pooled_pull_and_push_at_world_size_gt_1_on_one_gpu(dev, world, rows, width, B, ragged_odd):
    mp.spawn(_worker, args=(world, _free_port(), rows, width, B, ragged_odd), nprocs=world, join=True)
