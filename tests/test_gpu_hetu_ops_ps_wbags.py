"""The weighted pooled path of the plain PS flavour in herald_amd/hetu_ops.py (Config.ps_fuse_wbags): a communicate op that was
given bag= and next_weights= pulls weighted pooled rows (store.pull_wsum) and pushes weighted pooled slices as they are
(push_wbags).  Every item is checked against the same op with ps_fuse_wbags=False -- per-occurrence rows, the weighted summing
pass, the expanded gradient -- for bit-equal tables and pull buffers over 3 steps."""
import numpy as np
import pytest
import torch

from herald_amd import hetu_ops, ops
from herald_amd.sharded import ShardedEmbedding

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR, STEPS = 3000, 64, 24, 26, 0.05, 3


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


def _data(dev):
    """STEPS + 1 batches of FAE data: (cold ids [B, F], cold mask [B, F]) -- a dead slot names the padding id 0 -- and the
    gradients of the pooled rows; general weights on the last batch's twin are not needed: the mask is what FAE has."""
    rng = np.random.default_rng(77)
    table = rng.standard_normal((ROWS, WIDTH)).astype(np.float32)
    batches = []
    for _ in range(STEPS + 1):
        ids = rng.integers(1, ROWS, (B, F)).astype(np.float32)
        ids[:, :2] = ids[0, :2]
        w = rng.standard_normal((B, F)).astype(np.float32)      # general weights: the roundings of w * g show
        dead = rng.random((B, F)) < 0.5
        ids[dead], w[dead] = 0, 0
        batches.append((torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev)))
    grads = [torch.from_numpy(rng.standard_normal((B, WIDTH)).astype(np.float32)).to(dev) for _ in range(STEPS)]
    return table, batches, grads


def _run(dev, fuse, bsp, prefetch=True):
    """STEPS steps of lookup -> gradient -> communicate op; returns (table, the lookup's outputs, config, op)."""
    table, batches, grads = _data(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(table.copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = hetu_ops.Config(comm_mode="PS", bsp=bsp, prefetch=prefetch, ps_fuse_wbags=fuse)
    state = {"k": 0}
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[state["k"] + 1][0], bag=F,
                                                 next_weights=lambda: batches[state["k"] + 1][1])
    comm.forward_hook(cfg, first_ids=batches[0][0], first_weights=batches[0][1])
    look = hetu_ops.EmbeddingLookUpWeightedSum(param)
    look.forward_hook(cfg)
    look_grad = hetu_ops.EmbeddingLookUpWeightedSum_Gradient(param.shape)
    w_before = [b[1].clone() for b in batches]
    outs = []
    for k in range(STEPS):
        state["k"] = k
        ids, w = batches[k]
        out = torch.empty((B, WIDTH), dtype=torch.float32, device=dev)
        look.compute(ids, w, out)
        outs.append(out)
        g = grads[k].clone()
        comm.compute(look_grad.compute(g, ids, w))
        torch.cuda.synchronize()
        if fuse:      # -lr goes into the push: the caller's values and weights are as they were
            assert np.array_equal(_bits(g), _bits(grads[k])) and np.array_equal(_bits(w), _bits(w_before[k]))
    torch.cuda.synchronize()
    return store.table, outs, cfg, comm, param


@pytest.mark.parametrize("bsp", [-1, 0])          # asp (push_pull) and bsp / ssp (push, barrier, pull)
def test_communicate_op_with_bag_and_next_weights(dev, bsp):
    t_f, outs_f, cfg_f, comm_f, param_f = _run(dev, True, bsp)
    t_u, outs_u, cfg_u, comm_u, param_u = _run(dev, False, bsp)
    assert cfg_f.ps_wpooled.get(param_f) == F and not cfg_f.ps_pooled
    assert not cfg_u.ps_wpooled and not cfg_u.ps_pooled
    assert tuple(comm_f.sparse_pull_val.shape) == (B, WIDTH) and tuple(comm_u.sparse_pull_val.shape) == (B, F, WIDTH)
    for a, b in zip(outs_f, outs_u):
        assert np.array_equal(_bits(a), _bits(b)) and np.any(_bits(a))
    assert np.array_equal(_bits(t_f), _bits(t_u))
    table0 = _data(dev)[0]
    assert not np.array_equal(_bits(t_f), table0.view(np.int32))
    # the buffer pulled last: the weighted pooled rows of batch STEPS, which the unfused op holds per occurrence
    _, batches, _ = _data(dev)
    ids, w = batches[STEPS]
    pos = torch.arange(B * F, dtype=torch.int64, device=dev).view(B, F)
    want = ops.embedding_lookup_wsum(comm_u.sparse_pull_val.reshape(-1, WIDTH), pos, w)
    assert np.array_equal(_bits(comm_f.sparse_pull_val), _bits(want))


def test_the_lookup_without_prefetch_goes_through_pull_wsum(dev, monkeypatch):
    calls = []
    orig = ShardedEmbedding.pull_wsum

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    monkeypatch.setattr(ShardedEmbedding, "pull_wsum", spy)
    t_f, outs_f, _, _, _ = _run(dev, True, 0, prefetch=False)
    assert len(calls) == STEPS
    t_u, outs_u, _, _, _ = _run(dev, False, 0, prefetch=False)
    assert len(calls) == STEPS
    for a, b in zip(outs_f, outs_u):
        assert np.array_equal(_bits(a), _bits(b)) and np.any(_bits(a))
    assert np.array_equal(_bits(t_f), _bits(t_u))


def test_ragged_weighted_slices_stay_pooled(dev):
    """Ragged weighted slices that carry their offsets are pushed pooled by an op on the weighted PS path."""
    table, batches, grads = _data(dev)
    ids, w = batches[0][0].reshape(-1), batches[0][1].reshape(-1)
    n = ids.numel()
    cuts = np.sort(np.random.default_rng(3).integers(0, n + 1, B - 1))
    off = torch.from_numpy(np.concatenate([[0], cuts, [n]]).astype(np.int64)).to(dev)
    tables = []
    for fuse in (True, False):
        store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(table.copy()).to(dev))
        param = hetu_ops.EmbeddingParameter(store=store)
        cfg = hetu_ops.Config(comm_mode="PS", bsp=0, prefetch=False, ps_fuse_wbags=fuse)
        comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[1][0], bag=F,
                                                     next_weights=lambda: batches[1][1])
        comm.forward_hook(cfg)
        grad = hetu_ops.EmbeddingLookUpWeightedSum_Gradient(param.shape).compute(grads[0].clone(), ids, w, offsets=off)
        kept = comm._per_occurrence(grad)
        assert (kept is grad) == fuse
        comm.compute(grad)
        torch.cuda.synchronize()
        tables.append(_bits(store.table).copy())
    assert np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[0], table.view(np.int32))


def test_the_cache_flavour_refuses_next_weights(dev):
    _, batches, _ = _data(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev)
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=True, cstable_policy="LRU", cache_limit=B * F)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[1][0], bag=F,
                                                 next_weights=lambda: batches[1][1])
    with pytest.raises(ValueError, match="next_weights"):
        comm.forward_hook(cfg, first_ids=batches[0][0], first_weights=batches[0][1])


def test_weighted_fm_slices_are_refused(dev):
    _, batches, grads = _data(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev)
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = hetu_ops.Config(comm_mode="PS", bsp=0, prefetch=True)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[1][0], bag=F,
                                                 next_weights=lambda: batches[1][1])
    comm.forward_hook(cfg, first_ids=batches[0][0], first_weights=batches[0][1])
    ids, w = batches[0]
    grad = hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient(param.shape).compute(grads[0], grads[1], ids, w)
    before = _bits(store.table).copy()
    with pytest.raises(ValueError, match="FM-pooled"):
        comm.compute(grad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(store.table), before)


def test_first_ids_come_with_first_weights(dev):
    _, batches, _ = _data(dev)
    param = hetu_ops.EmbeddingParameter(store=ShardedEmbedding(ROWS, WIDTH, dev))
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[1][0], bag=F,
                                                 next_weights=lambda: batches[1][1])
    with pytest.raises(ValueError, match="first_weights"):
        comm.forward_hook(hetu_ops.Config(comm_mode="PS", bsp=0, prefetch=True), first_ids=batches[0][0])
