"""The weighted pooled path of the cache flavour in herald_amd/hetu_ops.py (Config.cache_fuse_wbags, opt-in): at bsp 0 with
prefetch, cache_plan_ahead and peek_ids on one rank, a communicate op that was given bag= and next_weights= pulls weighted pooled
rows (embedding_lookup_wsum_planned) and pushes the weighted pooled slices as they are, -lr included
(embedding_update_planned_wbags).  Held to the same loop whose op is built without bag= / next_weights=: per-occurrence planned
pairs, EmbeddingLookUpWeightedSum over the row buffer, unweighted_slices + scale_ -- bit-equal outputs, store and cache state."""
import gc

import numpy as np
import pytest
import torch

from herald_amd import cache as hcache
from herald_amd import hetu_ops
from herald_amd.sharded import ShardedEmbedding

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR, STEPS = 3000, 16, 24, 26, 0.05, 4


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)
    gc.collect()


def _bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _data(dev):
    """STEPS + 2 batches of FAE data -- a dead slot names the padding id 0, some dead slots keep their id with weight -0.0f --
    and the gradients of the pooled rows; general live weights, so the roundings of w * g show."""
    rng = np.random.default_rng(78)
    table = rng.standard_normal((ROWS, WIDTH)).astype(np.float32)
    batches = []
    for _ in range(STEPS + 2):
        ids = rng.integers(1, ROWS, (B, F)).astype(np.float32)
        ids[:, :2] = ids[0, :2]
        w = rng.standard_normal((B, F)).astype(np.float32)
        dead = rng.random((B, F)) < 0.5
        ids[dead], w[dead] = 0, 0
        w[rng.random((B, F)) < 0.05] = -0.0
        batches.append((torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev)))
    grads = [torch.from_numpy(rng.standard_normal((B, WIDTH)).astype(np.float32)).to(dev) for _ in range(STEPS)]
    return table, batches, grads


def _config(policy, fuse, **kw):
    args = dict(comm_mode="Hybrid", bsp=0, prefetch=True, cstable_policy=policy, cache_bound=1, cache_limit=700,
                cache_plan_ahead=True, cache_fuse_wbags=fuse)
    args.update(kw)
    return hetu_ops.Config(**args)


def _run(dev, policy, fuse):
    table, batches, grads = _data(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(table.copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = _config(policy, fuse)
    state = {"k": 0}

    def peek(j):
        k = state["k"] + 1 + j
        return batches[k][0] if k < len(batches) else None

    kw = dict(bag=F, next_weights=lambda: batches[state["k"] + 1][1]) if fuse else {}
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[state["k"] + 1][0], peek_ids=peek, **kw)
    if fuse:
        comm.forward_hook(cfg, first_ids=batches[0][0], first_weights=batches[0][1])
    else:
        comm.forward_hook(cfg, first_ids=batches[0][0])
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


@pytest.mark.parametrize("policy", ["LRU", "LFU"])
def test_communicate_op_with_cache_fuse_wbags(dev, policy, monkeypatch):
    calls = {"embedding_lookup_wsum_planned": 0, "embedding_update_planned_wbags": 0, "embedding_lookup_planned": 0,
             "embedding_update_planned": 0}
    for name in calls:
        def spy(self, *a, _orig=getattr(hcache.CacheSparseTable, name), _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(hcache.CacheSparseTable, name, spy)
    t_f, outs_f, cfg_f, comm_f, param_f = _run(dev, policy, True)
    assert calls == {"embedding_lookup_wsum_planned": STEPS + 1, "embedding_update_planned_wbags": STEPS,
                     "embedding_lookup_planned": 0, "embedding_update_planned": 0}
    assert comm_f._bag == F and comm_f._cache_wbags
    assert cfg_f.ps_wpooled.get(param_f) == F and not cfg_f.ps_pooled
    assert tuple(comm_f.sparse_pull_val.shape) == (B, WIDTH)
    for name in calls:
        calls[name] = 0
    t_u, outs_u, cfg_u, comm_u, param_u = _run(dev, policy, False)
    assert calls == {"embedding_lookup_wsum_planned": 0, "embedding_update_planned_wbags": 0,
                     "embedding_lookup_planned": STEPS + 1, "embedding_update_planned": STEPS}
    assert not cfg_u.ps_wpooled and not cfg_u.ps_pooled and tuple(comm_u.sparse_pull_val.shape) == (B, F, WIDTH)
    for k, (a, b) in enumerate(zip(outs_f, outs_u)):
        assert np.array_equal(_bits(a), _bits(b)) and np.any(_bits(a)), "output of step %d" % k
    assert np.array_equal(_bits(t_f), _bits(t_u)), "the store's table"
    table0 = _data(dev)[0]
    assert not np.array_equal(_bits(t_f), table0.view(np.int32))
    # the cache's state: resident keys, versions, update counters, data and gradient rows
    la, lb = comm_f.cache.cache.lines(), comm_u.cache.cache.lines()
    assert sorted(la) == sorted(lb)
    for key in la:
        assert la[key].version == lb[key].version and la[key].updates == lb[key].updates, key
        assert np.array_equal(_bits(la[key].data), _bits(lb[key].data)), key
        assert np.array_equal(_bits(la[key].grad), _bits(lb[key].grad)), key
    # the buffer pulled last: the weighted pooled rows of batch STEPS, which the unfused op holds per occurrence
    from herald_amd import ops
    _, batches, _ = _data(dev)
    pos = torch.arange(B * F, dtype=torch.int64, device=dev).view(B, F)
    want = ops.embedding_lookup_wsum(comm_u.sparse_pull_val.reshape(-1, WIDTH), pos, batches[STEPS][1])
    assert np.array_equal(_bits(comm_f.sparse_pull_val), _bits(want))


def _op(dev, cfg, bag=F, weights=True, peek=True, ids_shape=None):
    _, batches, _ = _data(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev)
    param = hetu_ops.EmbeddingParameter(store=store)
    kw = dict(next_weights=lambda: batches[1][1]) if weights else {}
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: batches[1][0],
                                                 peek_ids=(lambda j: batches[1 + j][0]) if peek else None, bag=bag, **kw)
    return comm, param, batches


def test_first_ids_come_with_first_weights(dev):
    comm, _, batches = _op(dev, None)
    with pytest.raises(ValueError, match="first_weights"):
        comm.forward_hook(_config("LRU", True), first_ids=batches[0][0])


def test_a_wrong_bag_size_is_refused(dev):
    comm, _, batches = _op(dev, None, bag=F + 1)
    with pytest.raises(ValueError, match="bag"):
        comm.forward_hook(_config("LRU", True), first_ids=batches[0][0], first_weights=batches[0][1])


def test_slices_that_are_not_the_weighted_ones_of_the_bag_are_refused(dev):
    _, _, grads = _data(dev)
    comm, param, batches = _op(dev, None)
    comm.forward_hook(_config("LFU", True), first_ids=batches[0][0], first_weights=batches[0][1])
    ids, w = batches[0]
    before = _bits(param.store.table).copy()
    with pytest.raises(RuntimeError, match="cache_fuse_wbags"):       # sum-pooled slices carry no weights
        comm.compute(hetu_ops.EmbeddingLookUpSum_Gradient(param.shape).compute(grads[0].clone(), ids))
    with pytest.raises(RuntimeError, match="cache_fuse_wbags"):       # per-occurrence slices
        comm.compute(hetu_ops.EmbeddingLookUp_Gradient(param.shape).compute(
            torch.zeros((B, F, WIDTH), dtype=torch.float32, device=dev), ids))
    with pytest.raises(RuntimeError, match="cache_fuse_wbags"):       # weighted, another bag size
        half = hetu_ops.EmbeddingLookUpWeightedSum_Gradient(param.shape).compute(
            torch.zeros((2 * B, WIDTH), dtype=torch.float32, device=dev), ids.reshape(2 * B, F // 2), w.reshape(2 * B, F // 2))
        comm.compute(half)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(param.store.table), before)


@pytest.mark.parametrize("how", ["off", "bsp", "no_prefetch", "no_plan_ahead", "no_peek"])
def test_every_other_cache_configuration_refuses_next_weights(dev, how):
    comm, _, batches = _op(dev, None, peek=how != "no_peek")
    cfg = {"off": _config("LRU", False), "bsp": _config("LRU", True, bsp=-1), "no_prefetch": _config("LRU", True, prefetch=False),
           "no_plan_ahead": _config("LRU", True, cache_plan_ahead=False), "no_peek": _config("LRU", True)}[how]
    with pytest.raises(ValueError, match="next_weights.*cache_fuse_wbags"):
        comm.forward_hook(cfg, first_ids=batches[0][0], first_weights=batches[0][1])
