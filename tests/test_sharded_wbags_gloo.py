"""Routing and plumbing of ShardedEmbedding.pull_wsum / push_wbags / push_pull_wbags under gloo (CPU, world sizes 2 and 3).

The arithmetic is a test double: tests/cpu_engine.CpuEngine plus the numpy chains of tests/wshard_model.py for the two weighted
end steps (expand_wsum, reduce_scaled_wbags).  What is under test is that the weighted pooled calls route, exchange, apply and
account exactly as pull / push do: pooled rows against tests/wbag_model.py on the global table, tables and stats against a twin
store driven through pull / push of the expanded values (wbag_model.wbag_grad_rows)."""
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


def _wbag_engine():
    from cpu_engine import CpuEngine
    import wshard_model

    class WbagCpuEngine(CpuEngine):
        """CpuEngine with the weighted pooled end steps as float32 chains in position / occurrence order."""

        def expand_wsum(self, rows, plan, weights, bag=None, offsets=None, out=None):
            got = wshard_model.gather_wsum_u32keys(rows.numpy(), plan.inv, weights.numpy(), bag=bag,
                                                   offsets=offsets.numpy() if offsets is not None else None)
            got = torch.from_numpy(got)
            if out is not None:
                out.copy_(got)
                return out
            return got

        def reduce_scaled_wbags(self, plan, bag_values, weights, scale, bag=None, bag_of=None, offsets=None):
            which = wshard_model.which_of(plan.n, bag=bag, offsets=offsets.numpy() if offsets is not None else None) \
                if bag_of is None else np.asarray(bag_of)
            red = np.zeros((max(plan.n, 1), bag_values.shape[1]), dtype=np.float32)
            red[:plan.uniq.size] = wshard_model.dedup_reduce_wbags(plan.inv, plan.uniq.size, bag_values.numpy(),
                                                                   weights.numpy(), which, scale)
            return torch.from_numpy(red)

    return WbagCpuEngine()


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
    import wbag_model
    import wshard_model
    from herald_amd.sharded import ShardedEmbedding, partition

    n = B * F
    rng = np.random.default_rng(2718)              # the same stream on every rank
    table_g = rng.standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)

    def store():
        return ShardedEmbedding(rows, width, "cpu", engine=_wbag_engine(),
                                table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()))

    emb, twin = store(), store()
    lr = 0.05

    def batch(step, r):
        """FAE data: half of the slots are dead and name the padding id 0; the live ones share keys between ranks."""
        g = np.random.default_rng(step * 100 + r)
        ids = g.integers(0, rows, size=n).astype(np.float32)
        ids[: n // 4] = np.random.default_rng(step).integers(0, rows, size=n // 4)     # keys shared between ranks
        w = g.standard_normal(n, dtype=np.float32)
        dead = g.random(n) < 0.5
        ids[dead], w[dead] = 0, 0
        w[0] = 1.5      # at least one live occurrence
        return ids, w

    def grads(step, r):
        return np.random.default_rng(7 + step * world + r).standard_normal((B, width), dtype=np.float32)

    def offs(step):
        return _offsets(n, B, step) if step % 2 else None      # ragged bags on odd steps

    def shaped(a, off):
        t = torch.from_numpy(a)
        return t if off is not None else t.view(B, F)

    def table_now():
        """The global table: every rank's shard of the twin store, gathered."""
        parts = [None] * world
        dist.all_gather_object(parts, twin.table.numpy().copy())
        return np.concatenate(parts)

    steps = 3
    ids0, _ = batch(0, rank)
    route = emb.prefetch(shaped(ids0, offs(0)), after_current=False)
    for k in range(steps):
        off = offs(k)
        t_off = torch.from_numpy(off) if off is not None else None
        cur = route
        if k + 1 < steps:
            route = emb.prefetch(shaped(batch(k + 1, rank)[0], offs(k + 1)), after_current=False)
        ids, w = batch(k, rank)
        want = table_now()
        got = emb.pull_wsum(weights=shaped(w, off), offsets=t_off, route=cur)       # one route: this pull and the push below
        ref = wbag_model.wbag_sum(want, ids if off is not None else ids.reshape(B, F), w if off is not None else w.reshape(B, F),
                                  off)
        np.testing.assert_array_equal(got.numpy().view(np.int32), ref.view(np.int32),
                                      err_msg="pull_wsum, step %d rank %d" % (k, rank))
        assert got.shape == (B, width) and np.any(got.numpy())
        twin.pull(torch.from_numpy(ids))
        g = grads(k, rank)
        t_g, t_w = torch.from_numpy(g.copy()), shaped(w.copy(), off)
        emb.push_wbags(None, t_g, t_w, lr, offsets=t_off, route=cur)
        np.testing.assert_array_equal(t_g.numpy().view(np.int32), g.view(np.int32))        # inputs as they were
        np.testing.assert_array_equal(t_w.numpy().reshape(-1).view(np.int32), w.view(np.int32))
        which = wshard_model.which_of(n, bag=F, offsets=off)
        before = twin.table.numpy().copy()
        twin.push(torch.from_numpy(ids), torch.from_numpy(wbag_model.wbag_grad_rows(g, w, which)), lr)
        if k + 1 < steps:
            emb.complete(route)
        dist.barrier()
        np.testing.assert_array_equal(emb.table.numpy().view(np.int32), twin.table.numpy().view(np.int32),
                                      err_msg="shard after push_wbags, step %d rank %d" % (k, rank))
        assert not np.array_equal(twin.table.numpy(), before)
        assert emb.stats == twin.stats

    # push_pull_wbags: every rank's push is applied (rank order) before any rank's pull is served
    off_push, off_pull = offs(9), offs(10)
    (ids_p, w_p), (ids_n, w_n) = batch(9, rank), batch(10, rank)
    g = grads(9, rank)
    got = emb.push_pull_wbags(shaped(ids_p, off_push), torch.from_numpy(g), shaped(w_p, off_push), lr, shaped(ids_n, off_pull),
                              shaped(w_n, off_pull),
                              push_offsets=torch.from_numpy(off_push) if off_push is not None else None,
                              pull_offsets=torch.from_numpy(off_pull) if off_pull is not None else None)
    which = wshard_model.which_of(n, bag=F, offsets=off_push)
    twin.push_pull(torch.from_numpy(ids_p), torch.from_numpy(wbag_model.wbag_grad_rows(g, w_p, which)), lr,
                   torch.from_numpy(ids_n))
    dist.barrier()
    want = table_now()
    ref = wbag_model.wbag_sum(want, ids_n if off_pull is not None else ids_n.reshape(B, F),
                              w_n if off_pull is not None else w_n.reshape(B, F), off_pull)
    np.testing.assert_array_equal(got.numpy().view(np.int32), ref.view(np.int32), err_msg="push_pull_wbags rows")
    np.testing.assert_array_equal(emb.table.numpy().view(np.int32), twin.table.numpy().view(np.int32))
    assert emb.stats == twin.stats and emb.stats["xgmi_bytes_out"] > 0

    # bad shapes are raised before the call's first collective: every rank raises, nobody waits in an exchange
    flat, wflat = torch.from_numpy(ids_p), torch.from_numpy(w_p)
    with pytest.raises(ValueError, match="offsets"):
        emb.pull_wsum(flat, wflat)
    with pytest.raises(ValueError, match="weights"):
        emb.pull_wsum(flat.view(B, F), wflat)                        # the weights do not have the ids' shape
    with pytest.raises(ValueError, match="weights"):
        emb.pull_wsum(flat.view(B, F), wflat.view(B, F).double())
    with pytest.raises(ValueError, match="bag_values"):
        emb.push_wbags(flat.view(B, F), torch.zeros((n, width)), wflat.view(B, F), lr)
    with pytest.raises(ValueError, match="weights"):
        emb.push_wbags(flat.view(B, F), torch.zeros((B, width)), None, lr)
    assert emb.stats == twin.stats
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,rows,width,B", [(2, 1001, 8, 12), (3, 500, 5, 9)])
def test_sharded_wbags_gloo(world, rows, width, B):
    mp.spawn(_worker, args=(world, _free_port(), rows, width, B), nprocs=world, join=True)
