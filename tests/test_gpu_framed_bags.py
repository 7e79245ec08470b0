"""FramedStep.pull_sum / push_bags / steps_bags on the HIP engine at world size 1: fixed frames replayed from hipGraphs, sized
eager launches, runs of steps by one native call (ha_shard_steps_bags).  Every pooled row equals FramedStep.pull on a twin store
followed by embedding_lookup_sum over the delivered rows, and the numpy position-ordered float32 chain over the oracle table
(tests/bag_model.py); every table equals, whole, the twin's after push of the expanded gradient and the oracle's serial PS
semantics (oracle/cpu.py sparse_push).  All comparisons on float32 bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
from test_gpu_framed import _stream  # noqa: E402
from test_gpu_shard_bags import _bits, _ragged_offsets  # noqa: E402

from herald_amd import ops  # noqa: E402
from oracle import cpu  # noqa: E402

pytestmark = pytest.mark.gpu


def _table(rows, width, seed=5):
    """Magnitudes over many binades, so that a change in the order of a sum shows."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, width), dtype=np.float32) * np.exp(rng.uniform(-6, 6, (rows, 1))).astype(np.float32))


class _Case:
    """A stream of batches with its bag layouts (batch k ragged where ragged(k)), pooled gradients and two stores: `emb` is
    driven through the pooled calls, `twin` through pull / push on the expanded gradient, `want` is the oracle's table."""

    def __init__(self, dev, rows, width, B, F, kind, nb, ragged, seed=0, int64_at=()):
        from herald_amd.sharded import ShardedEmbedding
        self.dev, self.rows, self.width, self.B, self.F, self.nb = dev, rows, width, B, F, nb
        self.ids = _stream(rows, B * F, nb, kind, seed)
        self.n = self.ids[0].size
        assert self.n == B * F
        self.offs = [_ragged_offsets(self.n, B, 100 + k) if ragged(k) else None for k in range(nb)]
        self.d_offs = [torch.from_numpy(o).to(dev) if o is not None else None for o in self.offs]
        rng = np.random.default_rng(seed + 15)
        self.g = [rng.standard_normal((B, width), dtype=np.float32) for _ in range(nb)]
        self.d_g = [torch.from_numpy(x).to(dev) for x in self.g]
        self.which = [np.arange(self.n) // F if o is None else bag_model.bag_of(o, self.n) for o in self.offs]
        self.d_exp = [torch.from_numpy(self.g[k][self.which[k]]).to(dev) for k in range(nb)]
        self.d_flat = []
        for k in range(nb):
            x = self.ids[k].astype(np.int64) if k in int64_at else self.ids[k]
            self.d_flat.append(torch.from_numpy(x).to(dev))
        table = _table(rows, width)
        self.want = table.copy()
        self.emb = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table.copy()).to(dev))
        self.twin = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table.copy()).to(dev))
        self.d_pos = torch.arange(self.n, dtype=torch.float32, device=dev)

    def staged(self, k):
        """Batch k as the pooled FramedStep is given it: [B, F] for fixed bags, [n] for ragged ones."""
        if k >= self.nb:
            return None
        return self.d_flat[k] if self.offs[k] is not None else self.d_flat[k].view(self.B, self.F)

    def flat(self, k):
        return self.d_flat[k] if k < self.nb else None

    def check_pooled_rows(self, k, got, delivered):
        """got = the pooled rows of batch k (table state: self.want); delivered = the twin's unpooled rows."""
        off = self.offs[k]
        assert got.shape == (self.B, self.width)
        ref = bag_model.bag_sum(self.want, self.ids[k] if off is not None else self.ids[k].reshape(self.B, self.F), off)
        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg="pull_sum of step %d" % k)
        d = delivered.reshape(self.n, self.width)
        summed = ops.embedding_lookup_sum(d, self.d_pos if off is not None else self.d_pos.view(self.B, self.F),
                                          offsets=self.d_offs[k])
        np.testing.assert_array_equal(_bits(got), _bits(summed), err_msg="pull + sum of step %d" % k)

    def oracle_push(self, k, lr):
        cpu.sparse_push(self.want, self.ids[k], self.g[k][self.which[k]], lr)

    def check_tables(self, k, oracle=True):
        torch.cuda.synchronize()
        a = self.emb.table.view(torch.int32)
        assert torch.equal(a, self.twin.table.view(torch.int32)), "table against push of the expanded gradient, step %d" % k
        if oracle:
            np.testing.assert_array_equal(_bits(self.emb.table), _bits(self.want), err_msg="table after step %d" % k)


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("rows,width,B,F,kind,graphs,block", [(3000, 64, 100, 9, "mixed", True, 2), (3000, 64, 100, 9, "mixed", False, 2),
                                                              (200, 32, 5, 8, "mixed", True, 1), (200, 32, 5, 8, "mixed", False, 1),
                                                              (50000, 128, 256, 26, "criteo", True, 4),
                                                              (50000, 128, 256, 26, "criteo", False, 4)])
def test_framed_bags_world1(dev, rows, width, B, F, kind, graphs, block, ragged):
    """graphs=True: fixed frames, pull_sum and push_bags of every step replay from hipGraphs; graphs=False: sized, one pooled
    launch each way.  Steps 3, 7, ... pull unpooled and push pooled, steps 5, 9, ... the reverse: the calls mix freely.  Batches
    2 and 6 are int64-keyed: they go through the pooled launches (neither overflows, `fallbacks` stays 0)."""
    from herald_amd.sharded import FramedStep
    nb = 9 * block + 3
    c = _Case(dev, rows, width, B, F, kind, nb, (lambda k: True) if ragged else (lambda k: False), int64_at=(2, 6))
    fs = FramedStep(c.emb, c.n, graphs=graphs, block=block)
    ft = FramedStep(c.twin, c.n, graphs=graphs, block=block)
    assert fs.sized == (not graphs)
    LA = fs.LOOKAHEAD
    fs.start([c.staged(k) for k in range(LA)])
    ft.start([c.flat(k) for k in range(LA)])
    outs = [torch.empty((B, width), device=dev) for _ in range(3)]
    # (a training loop keeps its offsets in a few buffers that it refills: the pointer is part of the key of a captured graph)
    obuf = [torch.zeros(B + 1, dtype=torch.int64, device=dev) for _ in range(3)]
    gbuf = [torch.zeros((B, width), device=dev) for _ in range(3)]
    lr = 0.05
    for k in range(nb):
        unpooled_pull, unpooled_push = k % 4 == 3, k % 4 == 1 and k > 1
        d_off = None
        if ragged:
            d_off = obuf[k % 3]
            d_off.copy_(c.d_offs[k])
        delivered = ft.pull(c.flat(k + LA))
        if unpooled_pull:
            got = fs.pull(c.staged(k + LA))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_bits(got).reshape(c.n, width), _bits(delivered).reshape(c.n, width))
        else:
            got = fs.pull_sum(c.staged(k + LA), offsets=d_off, out=outs[k % 3])
            assert got is outs[k % 3]
            torch.cuda.synchronize()
            c.check_pooled_rows(k, got, delivered)
        if unpooled_push:
            fs.push(c.d_exp[k], lr)
        else:
            gbuf[k % 3].copy_(c.d_g[k])
            fs.push_bags(gbuf[k % 3], lr, offsets=d_off)
        ft.push(c.d_exp[k], lr)
        c.oracle_push(k, lr)
        c.check_tables(k, oracle=rows <= 5000 or k == nb - 1)
    assert fs.fallbacks == 0 and fs.k == nb
    assert c.emb.stats == c.twin.stats
    if graphs:
        assert fs.graphs and sum(1 for g in fs._graphs.values() if g) >= 6, fs._graphs


@pytest.mark.parametrize("rows,width,B,F,kind,block,run", [(50000, 128, 256, 26, "criteo", 4, 4), (3000, 64, 100, 9, "mixed", 8, 3),
                                                           (200, 32, 5, 8, "mixed", 2, 2)])
def test_framed_steps_bags_by_one_native_call(dev, rows, width, B, F, kind, block, run):
    """steps_bags: runs of pooled steps inside one routing block by ONE library call (ha_shard_steps_bags), fixed and ragged
    batches in the same run, equal to pull_sum / push_bags step by step (the twin is driven that way, the tail of the stream
    too); a run across a block boundary raises and moves nothing.  Batches 1 (ragged) and 2 (fixed) are int64-keyed."""
    from herald_amd.sharded import FramedStep
    nb = 6 * block + 3
    c = _Case(dev, rows, width, B, F, kind, nb, lambda k: k % 2 == 1, seed=3, int64_at=(1, 2))
    fs = FramedStep(c.emb, c.n, graphs=False, block=block)
    ft = FramedStep(c.twin, c.n, graphs=False, block=block)
    assert fs.sized and fs.native_ok()
    LA = fs.LOOKAHEAD
    fs.start([c.staged(k) for k in range(LA)])
    ft.start([c.staged(k) for k in range(LA)])
    lr = 0.05
    k = 0
    while k < nb:
        cnt = 1 if k >= nb - 3 else min(run, nb - k, block - k % block)
        if k >= nb - 3:              # the tail of the stream: step by step
            got = [fs.pull_sum(c.staged(k + LA), offsets=c.d_offs[k])]
            fs.push_bags(c.d_g[k], lr, offsets=c.d_offs[k])
        else:
            outs = [torch.empty((B, width), device=dev) for _ in range(cnt)]
            got = fs.steps_bags([c.staged(k + i + LA) for i in range(cnt)], c.d_g[k:k + cnt], lr, outs=outs,
                                offsets_list=c.d_offs[k:k + cnt])
            assert all(a is b for a, b in zip(got, outs))
            # the run went to the library as one call (the step-by-step fallback would give the same rows and keeps nothing)
            assert getattr(fs, "_keep", (None, None))[1] is outs and fs.k == k + cnt
        torch.cuda.synchronize()
        for i in range(cnt):
            tw = ft.pull_sum(c.staged(k + i + LA), offsets=c.d_offs[k + i])
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_bits(got[i]), _bits(tw), err_msg="rows of batch %d" % (k + i))
            off = c.offs[k + i]
            ref = bag_model.bag_sum(c.want, c.ids[k + i] if off is not None else c.ids[k + i].reshape(B, F), off)
            np.testing.assert_array_equal(_bits(got[i]), _bits(ref), err_msg="chain of batch %d" % (k + i))
            ft.push_bags(c.d_g[k + i], lr, offsets=c.d_offs[k + i])
            c.oracle_push(k + i, lr)
        k += cnt
    c.check_tables(nb - 1)
    assert fs.fallbacks == 0
    fs2 = FramedStep(c.emb, c.n, graphs=False, block=2)
    fs2.start([c.staged(k) for k in range(fs2.LOOKAHEAD)])
    with pytest.raises(ValueError, match="boundary"):
        fs2.steps_bags([None] * 3, c.d_g[:3], lr, offsets_list=c.d_offs[:3])     # three steps from step 0: blocks of 2
    assert fs2.k == 0 and not fs2._pending


def test_framed_bags_overflow_takes_the_sized_exchange(dev):
    """row_cap below the number of unique keys: the batch takes ShardedEmbedding.pull_sum / push_bags for itself, counted in
    `fallbacks`; results are unchanged.  One batch of the stream is int64-keyed."""
    from herald_amd.sharded import FramedStep
    rows, width, B, F, nb = 5000, 64, 48, 25, 6
    c = _Case(dev, rows, width, B, F, "mixed", nb, lambda k: k % 2 == 1, seed=3, int64_at=(4,))
    c.ids[1][:] = c.ids[1][0]                      # one unique key: fits any frame
    c.d_flat[1] = torch.from_numpy(c.ids[1]).to(dev)
    fs = FramedStep(c.emb, c.n, row_cap=64, block=2)
    ft = FramedStep(c.twin, c.n, row_cap=64, block=2)
    LA = fs.LOOKAHEAD
    fs.start([c.staged(k) for k in range(LA)])
    ft.start([c.flat(k) for k in range(LA)])
    for k in range(nb):
        delivered = ft.pull(c.flat(k + LA))
        got = fs.pull_sum(c.staged(k + LA), offsets=c.d_offs[k])
        torch.cuda.synchronize()
        c.check_pooled_rows(k, got, delivered)
        fs.push_bags(c.d_g[k], 0.1, offsets=c.d_offs[k])
        ft.push(c.d_exp[k], 0.1)
        c.oracle_push(k, 0.1)
        c.check_tables(k)
    assert fs.fallbacks == nb - 1 == ft.fallbacks           # every batch but the one-key batch
    assert c.emb.stats == c.twin.stats


def test_framed_bags_errors_leave_the_step_where_it_was(dev):
    from herald_amd.sharded import FramedStep
    rows, width, B, F, nb = 200, 32, 5, 8, 4
    c = _Case(dev, rows, width, B, F, "mixed", nb, lambda k: k == 1)
    fs = FramedStep(c.emb, c.n, graphs=False, block=2)
    with pytest.raises(RuntimeError):
        fs.pull_sum(None)                                           # before start
    fs.start([c.staged(k) for k in range(nb)])
    before = c.emb.table.clone()
    i64 = lambda m: torch.zeros(m, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="ragged"):
        fs.pull_sum(None, offsets=i64(B + 1))                       # batch 0 was staged as [B, F]
    with pytest.raises(ValueError, match="out"):
        fs.pull_sum(None, out=torch.empty((B + 1, width), device=dev))
    with pytest.raises(ValueError, match="int64"):
        fs.pull_sum(None, offsets=torch.zeros(B + 1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="int64"):
        fs.pull_sum(None, offsets=torch.zeros(B + 1, dtype=torch.int64))       # on the host
    with pytest.raises(RuntimeError):
        fs.push_bags(c.d_g[0])                                      # nothing pulled
    assert fs.k == 0 and not fs._pending
    fs.pull_sum(None)
    with pytest.raises(ValueError, match="bag_values"):
        fs.push_bags(c.d_exp[0], 0.1)                               # the expanded gradient is not [B, width]
    with pytest.raises(ValueError, match="bag_values"):
        fs.push_bags(c.d_g[0].double(), 0.1)
    with pytest.raises(RuntimeError):
        fs.pull_sum(None)                                           # push first
    assert fs.k == 0 and fs._pending
    torch.cuda.synchronize()
    assert torch.equal(before, c.emb.table)
    fs.push_bags(c.d_g[0], 0.1)
    assert fs.k == 1
    with pytest.raises(ValueError, match="fixed bags"):
        fs.pull_sum(None)                                           # batch 1 was staged as [n]: it needs offsets
    with pytest.raises(ValueError):
        fs.steps_bags([None], [c.d_g[1]], 0.1)                      # the same through steps_bags
    with pytest.raises(ValueError, match="bag_values"):
        fs.steps_bags([None], [c.d_exp[1]], 0.1, offsets_list=[c.d_offs[1]])
    with pytest.raises(ValueError, match="outs"):
        fs.steps_bags([None], [c.d_g[1]], 0.1, outs=[torch.empty((B, width + 1), device=dev)], offsets_list=[c.d_offs[1]])
    assert fs.k == 1 and not fs._pending
    got = fs.steps_bags([None], [c.d_g[1]], 0.1, offsets_list=[c.d_offs[1]])
    assert fs.k == 2 and got[0].shape == (B, width)
    torch.cuda.synchronize()
