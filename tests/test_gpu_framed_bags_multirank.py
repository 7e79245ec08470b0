"""FramedStep.pull_sum / push_bags at world sizes 2 and 4 as W processes on one GPU (host-staged all-to-all, as in
test_gpu_framed.py), sized exchanges and fixed row frames: pooled rows against the numpy position-ordered chain over the
oracle's global table (tests/bag_model.py), shards against the oracle's serial rank-ordered PS semantics (oracle/cpu.py
sparse_push on the expanded gradients).  Float32 bit patterns throughout."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 13


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _staged(out, inp, out_splits, in_splits, group):
    torch.cuda.current_stream().synchronize()
    o = torch.empty(out.shape, dtype=out.dtype)
    dist.all_to_all_single(o, inp.cpu(), out_splits, in_splits, group=group)
    out.copy_(o)


def _worker(rank, world, port, rows, width, B, row_cap, expect_fallback, sized):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    import bag_model
    from herald_amd.sharded import FramedStep, ShardedEmbedding, partition
    from oracle import cpu
    from test_gpu_framed import _stream
    from test_gpu_shard_bags import _ragged_offsets
    rng = np.random.default_rng(77)
    table_g = (rng.standard_normal((rows, width), dtype=np.float32) * np.exp(rng.uniform(-6, 6, (rows, 1))).astype(np.float32))
    starts = partition(rows, world)
    emb = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table_g[starts[rank]:starts[rank + 1]].copy()).to(dev),
                           a2a=_staged)
    nb, n = 5, B * F
    streams = [_stream(rows, n, nb, "mixed", seed=10 + r) for r in range(world)]
    if world > 2:
        streams[world - 1][2] = streams[world - 1][2][:0]             # an empty batch on the last rank
    offs = [_ragged_offsets(n, B, 50 + k) if k % 2 else None for k in range(nb)]      # ragged bags on odd steps
    size = lambda r, k: streams[r][k].size
    bags = lambda r, k: size(r, k) // F if offs[k] is None else B
    grads = [[np.random.default_rng(500 + k * world + r).standard_normal((bags(r, k), width), dtype=np.float32)
              for r in range(world)] for k in range(nb)]

    def expanded(r, k):
        m = size(r, k)
        return grads[k][r][np.arange(m) // F] if offs[k] is None else grads[k][r][bag_model.bag_of(offs[k], m)]

    fs = FramedStep(emb, n, row_cap=row_cap, block=2, graphs=False, sized=sized)  # (a host-staged exchange cannot be captured)

    def tid(k):
        if k >= nb:
            return None
        t = torch.from_numpy(streams[rank][k]).to(dev)
        return t if offs[k] is not None else t.view(-1, F)

    LA = fs.LOOKAHEAD
    fs.start([tid(k) for k in range(LA)])
    want = table_g.copy()
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    for k in range(nb):
        d_off = torch.from_numpy(offs[k]).to(dev) if offs[k] is not None else None
        got = fs.pull_sum(tid(k + LA), offsets=d_off)
        torch.cuda.synchronize()
        mine = streams[rank][k]
        if mine.size:
            ref = bag_model.bag_sum(want, mine if offs[k] is not None else mine.reshape(-1, F), offs[k])
            np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(ref), err_msg="pull_sum, step %d rank %d" % (k, rank))
        else:
            assert got is None
        fs.push_bags(torch.from_numpy(grads[k][rank]).to(dev), 0.05, offsets=d_off)
        torch.cuda.synchronize()
        dist.barrier()
        for r in range(world):
            if size(r, k):
                cpu.sparse_push(want, streams[r][k], expanded(r, k), 0.05)
        np.testing.assert_array_equal(bits(emb.table.cpu().numpy()), bits(want[starts[rank]:starts[rank + 1]]),
                                      err_msg="shard after push_bags, step %d rank %d" % (k, rank))
    assert (fs.fallbacks > 0) == expect_fallback, fs.fallbacks
    if sized and not expect_fallback:
        # the row exchanges carried exactly the rows the batches name, as for pull / push
        st = np.asarray(starts)
        real = 0
        for k in range(nb):
            u = [np.unique(cpu.ids_to_keys(streams[r][k])).astype(np.int64) for r in range(world)]
            real += int(((u[rank] < st[rank]) | (u[rank] >= st[rank + 1])).sum())
            real += sum(int(((u[r] >= st[rank]) & (u[r] < st[rank + 1])).sum()) for r in range(world) if r != rank)
        assert emb.stats["xgmi_row_bytes"] == 2 * 4 * width * real
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,rows,width,B,row_cap,expect_fallback,sized",
                         [(2, 5000, 64, 100, 300, True, True), (2, 5000, 64, 100, None, False, True),
                          (4, 5000, 64, 100, None, False, True),
                          (2, 5000, 64, 100, None, False, False), (4, 5000, 66, 100, 200, True, False)])
def test_framed_bags_at_world_size_gt_1_on_one_gpu(dev, world, rows, width, B, row_cap, expect_fallback, sized):
    mp.spawn(_worker, args=(world, _free_port(), rows, width, B, row_cap, expect_fallback, sized), nprocs=world, join=True)
