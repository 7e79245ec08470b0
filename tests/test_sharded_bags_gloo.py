"""Routing and plumbing of ShardedEmbedding.pull_sum / push_bags / push_pull_bags under gloo (CPU, world sizes 2 and 3).

The arithmetic is a test double: tests/cpu_engine.CpuEngine plus numpy chains for the two pooled end steps (expand_sum,
reduce_scaled_bags).  What is under test is that the pooled calls route, exchange, apply and account exactly as pull / push
do: pooled rows against tests/bag_model.py on the global table, shards against the oracle's serial PS semantics
(oracle/cpu.py sparse_push, rank order, expanded values), tables and stats against a twin store driven through pull / push."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 26


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bag_engine():
    from cpu_engine import CpuEngine
    import bag_model

    class BagCpuEngine(CpuEngine):
        """CpuEngine with the pooled end steps as float32 chains in position / occurrence order."""

        def expand_sum(self, rows, plan, bag=None, offsets=None, out=None):
            inv = plan.inv.astype(np.int64)
            if offsets is None:
                got = bag_model.bag_sum(rows.numpy(), inv.reshape(-1, bag))
            else:
                got = bag_model.bag_sum(rows.numpy(), inv, offsets.numpy())
            got = torch.from_numpy(got)
            if out is not None:
                out.copy_(got)
                return out
            return got

        def reduce_scaled_bags(self, plan, bag_values, scale, bag=None, bag_of=None, offsets=None):
            if offsets is not None:
                bag_of = bag_model.bag_of(offsets.numpy(), plan.n)
            which = np.arange(plan.n) // bag if bag_of is None else np.asarray(bag_of)
            v = (bag_values.numpy() * np.float32(scale)).astype(np.float32)
            red = np.zeros((max(plan.n, 1), v.shape[1]), dtype=np.float32)
            for i, u in enumerate(plan.inv):
                red[u] = red[u] + v[which[i]]
            return torch.from_numpy(red)

    return BagCpuEngine()


def _offsets(n, nbags, seed):
    """Ragged bags with empty ones at the front, in the middle and at the end."""
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, nbags - 4))
    h = cuts.size // 2
    return np.concatenate([[0, 0], cuts[:h], [cuts[h]], cuts[h:], [n, n]]).astype(np.int64)


def _worker(rank, world, port, rows, width, B):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bag_model
    from herald_amd.sharded import ShardedEmbedding, partition
    from oracle import cpu

    n = B * F
    rng = np.random.default_rng(2718)              # the same stream on every rank
    table_g = rng.standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)

    def store():
        return ShardedEmbedding(rows, width, "cpu", engine=_bag_engine(),
                                table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()))

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
        return _offsets(n, B, step) if step % 2 else None      # ragged bags on odd steps

    def expanded(g, off):
        return g[np.arange(n) // F] if off is None else g[bag_model.bag_of(off, n)]

    def ids_t(step, r, off):
        t = torch.from_numpy(batch(step, r))
        return t if off is not None else t.view(B, F)

    steps = 3
    route = emb.prefetch(ids_t(0, rank, offs(0)), after_current=False)
    for k in range(steps):
        off = offs(k)
        t_off = torch.from_numpy(off) if off is not None else None
        cur = route
        if k + 1 < steps:
            route = emb.prefetch(ids_t(k + 1, rank, offs(k + 1)), after_current=False)
        got = emb.pull_sum(offsets=t_off, route=cur)
        ids = batch(k, rank)
        np.testing.assert_array_equal(got.numpy().view(np.int32),
                                      bag_model.bag_sum(want, ids if off is not None else ids.reshape(B, F), off).view(np.int32),
                                      err_msg="pull_sum, step %d rank %d" % (k, rank))
        assert got.shape == (B, width) and np.any(got.numpy())
        rows_t = twin.pull(torch.from_numpy(ids))
        np.testing.assert_array_equal(rows_t.numpy(), cpu.sparse_pull(want, ids))
        g = grads(k, rank)
        t_g = torch.from_numpy(g.copy())
        emb.push_bags(None, t_g, lr, offsets=t_off, route=cur)
        np.testing.assert_array_equal(t_g.numpy().view(np.int32), g.view(np.int32))        # inputs as they were
        twin.push(torch.from_numpy(ids), torch.from_numpy(expanded(g, off)), lr)
        if k + 1 < steps:
            emb.complete(route)
        dist.barrier()
        before = want[starts[rank]:starts[rank + 1]].copy()
        for r in range(world):                               # servers apply in rank order
            cpu.sparse_push(want, batch(k, r), expanded(grads(k, r), off), lr)
        shard = want[starts[rank]:starts[rank + 1]]
        np.testing.assert_array_equal(emb.table.numpy().view(np.int32), shard.view(np.int32),
                                      err_msg="shard after push_bags, step %d rank %d" % (k, rank))
        np.testing.assert_array_equal(emb.table.numpy().view(np.int32), twin.table.numpy().view(np.int32))
        assert not np.array_equal(shard, before)
        assert emb.stats == twin.stats

    # push_pull_bags: every rank's push is applied (rank order) before any rank's pull is served
    off_push, off_pull = offs(9), offs(10)
    g = grads(9, rank)
    got = emb.push_pull_bags(ids_t(9, rank, off_push), torch.from_numpy(g), lr, ids_t(10, rank, off_pull),
                             push_offsets=torch.from_numpy(off_push) if off_push is not None else None,
                             pull_offsets=torch.from_numpy(off_pull) if off_pull is not None else None)
    twin.push_pull(torch.from_numpy(batch(9, rank)), torch.from_numpy(expanded(g, off_push)), lr,
                   torch.from_numpy(batch(10, rank)))
    dist.barrier()
    for r in range(world):
        cpu.sparse_push(want, batch(9, r), expanded(grads(9, r), off_push), lr)
    nxt = batch(10, rank)
    np.testing.assert_array_equal(got.numpy().view(np.int32),
                                  bag_model.bag_sum(want, nxt if off_pull is not None else nxt.reshape(B, F),
                                                    off_pull).view(np.int32), err_msg="push_pull_bags rows")
    np.testing.assert_array_equal(emb.table.numpy().view(np.int32), want[starts[rank]:starts[rank + 1]].view(np.int32))
    np.testing.assert_array_equal(emb.table.numpy().view(np.int32), twin.table.numpy().view(np.int32))
    assert emb.stats == twin.stats and emb.stats["xgmi_bytes_out"] > 0

    # shape errors are raised before the call's first collective: every rank raises, nobody waits in an exchange
    flat = torch.from_numpy(batch(0, rank))
    with pytest.raises(ValueError, match="offsets"):
        emb.pull_sum(flat)
    with pytest.raises(ValueError, match="bag_values"):
        emb.push_bags(flat.view(B, F), torch.zeros((n, width)), lr)
    with pytest.raises(ValueError, match="int64"):
        emb.pull_sum(flat, offsets=torch.zeros(B + 1, dtype=torch.int32))
    assert emb.stats == twin.stats
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,rows,width,B", [(2, 1001, 8, 12), (3, 500, 5, 9)])
def test_sharded_bags_gloo(world, rows, width, B):
    mp.spawn(_worker, args=(world, _free_port(), rows, width, B), nprocs=world, join=True)
