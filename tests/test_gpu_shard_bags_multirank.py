"""ShardedEmbedding.pull_sum / push_bags / push_pull_bags with the HIP engine at world sizes 2 and 4 on ONE GPU, in the manner
of tests/test_gpu_sharded_multirank.py: every rank is a process with its own shard on cuda:0, the collectives run on a gloo
group and the buffers are staged through the host for them (the store's `a2a` hook).  Pooled rows against tests/bag_model.py on
the global table, shards against the oracle's serial PS semantics (oracle/cpu.py sparse_push in rank order, expanded values),
tables and stats against a twin store driven through pull / push in the same workers.  Bit patterns throughout."""
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
    import bag_model
    from herald_amd.sharded import ShardedEmbedding, partition
    from oracle import cpu

    n = B * F
    rng = np.random.default_rng(4321)              # the same stream on every rank
    table_g = rng.standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)

    def store():
        return ShardedEmbedding(rows, width, dev, a2a=host_staged_a2a,
                                table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()).to(dev))

    emb, twin = store(), store()
    want = table_g.copy()
    lr = 0.05

    def batch(step, r):
        g = np.random.default_rng(step * 100 + r)
        ids = g.integers(0, rows, size=n).astype(np.float32)
        ids[: n // 4] = np.random.default_rng(step).integers(0, rows, size=n // 4)     # keys shared between ranks
        ids[n // 4: n // 3] = ids[0]                                                   # a long run inside a rank
        return ids

    def grads(step, r):
        return np.random.default_rng(7 + step * world + r).standard_normal((B, width), dtype=np.float32)

    def offs(step):
        return _offsets(n, B, step) if ragged_odd and step % 2 else None

    def expanded(g, off):
        return g[np.arange(n) // F] if off is None else g[bag_model.bag_of(off, n)]

    def ids_t(step, r, off):
        t = torch.from_numpy(batch(step, r)).to(dev)
        return t if off is not None else t.view(B, F)

    def pooled(table, ids, off):
        return bag_model.bag_sum(table, ids if off is not None else ids.reshape(B, F), off)

    steps = 3
    route = emb.prefetch(ids_t(0, rank, offs(0)), after_current=False)
    for k in range(steps):
        off = offs(k)
        d_off = torch.from_numpy(off).to(dev) if off is not None else None
        cur = route
        if k + 1 < steps:
            route = emb.prefetch(ids_t(k + 1, rank, offs(k + 1)), after_current=False)
        got = emb.pull_sum(offsets=d_off, route=cur)
        torch.cuda.synchronize()
        ids = batch(k, rank)
        assert got.shape == (B, width)
        np.testing.assert_array_equal(_bits(got), _bits(pooled(want, ids, off)), err_msg="pull_sum, step %d rank %d" % (k, rank))
        assert np.any(_bits(got))
        d_flat = torch.from_numpy(ids).to(dev)
        np.testing.assert_array_equal(_bits(twin.pull(d_flat)), _bits(cpu.sparse_pull(want, ids)))
        g = grads(k, rank)
        d_g = torch.from_numpy(g).to(dev)
        emb.push_bags(None, d_g, lr, offsets=d_off, route=cur)
        twin.push(d_flat, torch.from_numpy(expanded(g, off)).to(dev), lr)
        if k + 1 < steps:
            emb.complete(route)
        torch.cuda.synchronize()
        dist.barrier()
        np.testing.assert_array_equal(_bits(d_g), _bits(g))                 # inputs as they were
        before = want[starts[rank]:starts[rank + 1]].copy()
        for r in range(world):                               # servers apply in rank order
            cpu.sparse_push(want, batch(k, r), expanded(grads(k, r), off), lr)
        shard = want[starts[rank]:starts[rank + 1]]
        np.testing.assert_array_equal(_bits(emb.table), _bits(shard), err_msg="shard after push_bags, step %d rank %d" % (k, rank))
        np.testing.assert_array_equal(_bits(emb.table), _bits(twin.table))
        assert not np.array_equal(_bits(shard), _bits(before))
        assert emb.stats == twin.stats

    # push_pull_bags: every rank's push is applied (rank order) before any rank's pull is served
    off_push, off_pull = offs(9), offs(10)
    g = grads(9, rank)
    got = emb.push_pull_bags(ids_t(9, rank, off_push), torch.from_numpy(g).to(dev), lr, ids_t(10, rank, off_pull),
                             push_offsets=torch.from_numpy(off_push).to(dev) if off_push is not None else None,
                             pull_offsets=torch.from_numpy(off_pull).to(dev) if off_pull is not None else None)
    twin.push_pull(torch.from_numpy(batch(9, rank)).to(dev), torch.from_numpy(expanded(g, off_push)).to(dev), lr,
                   torch.from_numpy(batch(10, rank)).to(dev))
    torch.cuda.synchronize()
    dist.barrier()
    for r in range(world):
        cpu.sparse_push(want, batch(9, r), expanded(grads(9, r), off_push), lr)
    np.testing.assert_array_equal(_bits(got), _bits(pooled(want, batch(10, rank), off_pull)), err_msg="push_pull_bags rows")
    np.testing.assert_array_equal(_bits(emb.table), _bits(want[starts[rank]:starts[rank + 1]]))
    np.testing.assert_array_equal(_bits(emb.table), _bits(twin.table))
    assert emb.stats == twin.stats and emb.stats["xgmi_bytes_out"] > 0
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,rows,width,B,ragged_odd", [(2, 5000, 64, 50, False), (4, 20000, 33, 100, True)])
def test_pooled_pull_and_push_at_world_size_gt_1_on_one_gpu(dev, world, rows, width, B, ragged_odd):
    mp.spawn(_worker, args=(world, _free_port(), rows, width, B, ragged_odd), nprocs=world, join=True)
