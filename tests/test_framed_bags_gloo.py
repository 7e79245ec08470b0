"""Routing and plumbing of FramedStep.pull_sum / push_bags / steps_bags under gloo (CPU, world sizes 2 and 3).

The arithmetic is a test double: the CpuEngine of test_sharded_bags_gloo.py plus numpy chains for the pooled end steps of the
framed engine (the two-source bag sum, the sum over the row frames, the pooled reduces).  What is under test is that the pooled
calls route, exchange, fall back, apply and account exactly as pull / push do: pooled rows against tests/bag_model.py on the
global table, shards against the oracle's serial PS semantics (oracle/cpu.py sparse_push in rank order on the expanded
values), tables, `fallbacks` and `stats` against a twin store driven through FramedStep.pull / push."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _framed_bag_engine():
    import bag_model
    from test_sharded_bags_gloo import _bag_engine

    class FramedBagCpuEngine(type(_bag_engine())):
        """The pooled end steps of the framed engine as float32 chains in position / occurrence order."""

        @staticmethod
        def _chain(rows, fb, lay, out):
            lo, hi = bag_model.bag_bounds((lay.nbags, lay.bag) if lay.bag else fb.n,
                                          None if lay.bag else lay.offsets.numpy())
            o = out.numpy()
            for b in range(lay.nbags):
                acc = np.zeros(rows.shape[1], dtype=np.float32)
                for j in range(int(lo[b]), int(hi[b])):
                    acc = (acc + rows[j]).astype(np.float32)
                o[b] = acc

        def sized_expand_sum(self, table, rows_recv, fb, lay, out):
            rows = torch.zeros((max(fb.n, 1), table.shape[1]), dtype=torch.float32)
            self.sized_expand(table, rows_recv, fb, rows[:fb.n])
            self._chain(rows.numpy(), fb, lay, out)

        def frames_expand_sum(self, rows_recv, fb, lay, out):
            rows = torch.zeros((max(fb.n, 1), rows_recv.shape[1]), dtype=torch.float32)
            self.frames_expand(rows_recv, fb, rows[:fb.n])
            self._chain(rows.numpy(), fb, lay, out)

        def bag_of(self, lay, n):
            if lay.bag == 0 and n:
                lay.bag_of[:n] = torch.from_numpy(bag_model.bag_of(lay.offsets.numpy(), n))

        @staticmethod
        def _expanded(fb, bag_values, lay):
            which = np.arange(fb.n) // lay.bag if lay.bag else lay.bag_of[:fb.n].numpy()
            return torch.from_numpy(bag_values.numpy()[which])

        def sized_reduce_bags(self, fb, bag_values, scale, push_buf, zero_flags, lay):
            if fb.n:
                self.sized_reduce(fb, self._expanded(fb, bag_values, lay), scale, push_buf, zero_flags)

        def frames_reduce_bags(self, fb, bag_values, scale, rows_send, zero_flags, lay):
            if fb.n:
                self.frames_reduce(fb, self._expanded(fb, bag_values, lay), scale, rows_send, zero_flags)

        def sized_push_alone_bags(self, table, fb, bag_values, scale, lay):
            if fb.n:
                self.sized_push_alone(table, fb, self._expanded(fb, bag_values, lay), scale)

    return FramedBagCpuEngine()


def _offsets(n, nbags, seed):
    """Ragged bags with empty ones at the front, in the middle and at the end."""
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, nbags - 4))
    h = cuts.size // 2
    return np.concatenate([[0, 0], cuts[:h], [cuts[h]], cuts[h:], [n, n]]).astype(np.int64)


def _worker(rank, world, port, rows, width, B, row_cap, block, expect_fallback, sized):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bag_model
    from herald_amd.sharded import FramedStep, ShardedEmbedding, partition
    from oracle import cpu

    n = B * F
    rng = np.random.default_rng(4242)               # the same stream on every rank
    table_g = rng.standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)

    def store():
        return ShardedEmbedding(rows, width, "cpu", engine=_framed_bag_engine(),
                                table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()))

    emb, twin = store(), store()
    nb = 7
    batches, grads, offs = [], [], []
    for k in range(nb):
        per = []
        for r in range(world):
            m = n if not (k == 2 and r == world - 1) else 0           # one empty batch on the last rank
            ids = rng.integers(0, rows, size=m).astype(np.float32)
            if m:
                ids[: m // 4] = (np.arange(m // 4) * 3) % rows        # keys every rank names
                ids[m // 4: m // 3] = ids[0]                          # a run
            if k == 4 and m:                                          # many unique keys of ONE owner
                ids = rng.permutation(starts[1])[:m].astype(np.float32) if starts[1] >= m else ids % starts[1]
            per.append(ids)
        batches.append(per)
        grads.append([rng.standard_normal((b.size // F, width), dtype=np.float32) for b in per])
        offs.append(_offsets(n, B, k) if k % 2 else None)             # ragged bags on odd steps (full batches only)

    def expanded(k, r):
        m = batches[k][r].size
        return grads[k][r][np.arange(m) // F] if offs[k] is None else grads[k][r][bag_model.bag_of(offs[k], m)]

    def tid(k, pooled=True):
        if k >= nb:
            return None
        t = torch.from_numpy(batches[k][rank])
        return t.view(-1, F) if (pooled and offs[k] is None) else t

    fs = FramedStep(emb, n, row_cap=row_cap, block=block, graphs=False, sized=sized)
    ft = FramedStep(twin, n, row_cap=row_cap, block=block, graphs=False, sized=sized)
    LA = fs.LOOKAHEAD
    fs.start([tid(k) for k in range(min(LA, nb))])
    ft.start([tid(k, False) for k in range(min(LA, nb))])
    want = table_g.copy()
    lr = 0.05
    for k in range(nb):
        off = offs[k]
        t_off = torch.from_numpy(off) if off is not None else None
        ids = batches[k][rank]
        # errors are raised before anything moves: every rank raises, nobody waits in an exchange
        k_before = fs.k
        with pytest.raises(ValueError):
            fs.pull_sum(tid(k + LA), offsets=torch.zeros(B + 1, dtype=torch.int32) if off is not None else torch.zeros(3, dtype=torch.int64))
        assert fs.k == k_before and not fs._pending
        pooled_pull, pooled_push = k != 3, k != 6          # steps 3 and 6 mix a pooled and an unpooled half
        if pooled_pull:
            got = fs.pull_sum(tid(k + LA), offsets=t_off)
            if ids.size:
                ref = bag_model.bag_sum(want, ids if off is not None else ids.reshape(-1, F), off)
                np.testing.assert_array_equal(got.numpy().view(np.int32), ref.view(np.int32),
                                              err_msg="pull_sum, step %d rank %d" % (k, rank))
                assert got.shape == (B, width)
            else:
                assert got is None
        else:
            got = fs.pull(tid(k + LA))
            np.testing.assert_array_equal(got.numpy().reshape(-1, width), want[ids.astype(np.int64)])
        rows_t = ft.pull(tid(k + LA, False))
        if ids.size:
            np.testing.assert_array_equal(rows_t.numpy().reshape(-1, width), want[ids.astype(np.int64)])
        g = grads[k][rank]
        if pooled_push:
            with pytest.raises(ValueError, match="bag_values"):
                fs.push_bags(torch.zeros((B + 1, width)), lr, offsets=t_off)
            assert fs.k == k_before and fs._pending
            fs.push_bags(torch.from_numpy(g.copy()), lr, offsets=t_off)
        else:
            fs.push(torch.from_numpy(expanded(k, rank)), lr)
        ft.push(torch.from_numpy(expanded(k, rank)), lr)
        assert fs.k == k_before + 1
        dist.barrier()
        for r in range(world):                                        # rank order
            if batches[k][r].size:
                cpu.sparse_push(want, batches[k][r], expanded(k, r), lr)
        shard = want[starts[rank]:starts[rank + 1]]
        np.testing.assert_array_equal(emb.table.numpy().view(np.int32), shard.view(np.int32),
                                      err_msg="shard after push_bags, step %d rank %d" % (k, rank))
        np.testing.assert_array_equal(emb.table.numpy().view(np.int32), twin.table.numpy().view(np.int32))
        assert emb.stats == twin.stats, (k, emb.stats, twin.stats)
        assert fs.fallbacks == ft.fallbacks
    assert (fs.fallbacks > 0) == expect_fallback, fs.fallbacks
    assert emb.stats["xgmi_bytes_out"] > 0
    with pytest.raises(RuntimeError, match="ended"):
        fs.pull_sum(None)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,rows,width,B,row_cap,block,expect_fallback,sized",
                         [(2, 1001, 8, 24, None, 2, True, True),     # default row_cap: batch 4 overflows owner 0
                          (2, 1001, 8, 24, 120, 1, False, True),     # row_cap = n can never overflow; blocks of one batch
                          (3, 700, 4, 18, 40, 4, True, True),        # the stream ends inside a block
                          (3, 700, 4, 18, 90, 4, False, True),
                          (2, 1001, 8, 24, None, 2, True, False),    # fixed row frames (the graph-replay form)
                          (3, 700, 4, 18, 90, 4, False, False)])
def test_framed_bags_gloo(world, rows, width, B, row_cap, block, expect_fallback, sized):
    mp.spawn(_worker, args=(world, _free_port(), rows, width, B, row_cap, block, expect_fallback, sized), nprocs=world,
             join=True)


def _steps_worker(rank, world, port):
    """steps_bags without the native step (the CPU engine): the same fallback rules as steps -- step by step."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bag_model
    from herald_amd.sharded import FramedStep, ShardedEmbedding, partition
    from oracle import cpu
    rows, width, B = 400, 4, 8
    n = B * F
    table_g = np.random.default_rng(1).standard_normal((rows, width), dtype=np.float32)
    starts = partition(rows, world)
    emb = ShardedEmbedding(rows, width, "cpu", engine=_framed_bag_engine(),
                           table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()))
    nb = 4
    ids = [[np.random.default_rng(10 * k + r).integers(0, rows, size=n).astype(np.float32) for r in range(world)]
           for k in range(nb)]
    g = [[np.random.default_rng(77 + 10 * k + r).standard_normal((B, width), dtype=np.float32) for r in range(world)]
         for k in range(nb)]
    off = _offsets(n, B, 3)
    fs = FramedStep(emb, n, block=2, graphs=False)
    assert not fs.native_ok()
    tid = lambda k: (torch.from_numpy(ids[k][rank]).view(B, F) if k % 2 == 0 else torch.from_numpy(ids[k][rank])) \
        if k < nb else None
    fs.start([tid(k) for k in range(nb)])
    want = table_g.copy()
    for k0 in (0, 2):
        offs_l = [None, torch.from_numpy(off)]
        with pytest.raises(ValueError):
            fs.steps_bags([None] * 3, [torch.from_numpy(g[k0][rank])] * 3, 0.1, offsets_list=[None, offs_l[1], None])
        assert fs.k == k0
        got = fs.steps_bags([None, None], [torch.from_numpy(g[k0 + i][rank]) for i in range(2)], 0.1, offsets_list=offs_l)
        dist.barrier()
        for i in range(2):
            k = k0 + i
            ref = bag_model.bag_sum(want, ids[k][rank].reshape(B, F) if i == 0 else ids[k][rank], None if i == 0 else off)
            np.testing.assert_array_equal(got[i].numpy().view(np.int32), ref.view(np.int32))
            for r in range(world):
                ex = g[k][r][np.arange(n) // F] if i == 0 else g[k][r][bag_model.bag_of(off, n)]
                cpu.sparse_push(want, ids[k][r], ex, 0.1)
    np.testing.assert_array_equal(emb.table.numpy().view(np.int32), want[starts[rank]:starts[rank + 1]].view(np.int32))
    dist.barrier()
    dist.destroy_process_group()


def test_framed_steps_bags_gloo_falls_back_step_by_step():
    mp.spawn(_steps_worker, args=(2, _free_port()), nprocs=2, join=True)
