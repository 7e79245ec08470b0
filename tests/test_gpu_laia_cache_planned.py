"""ParameterServerCommunicateOp with Config.cache_plan_ahead on laia-scheduled batches: a batch that arrives as (ids, push plan)
is planned with its plan (ha_cache_plan_block_push_keys), its gradients go through embedding_update_planned -- and everything
equals the call-by-call run (embedding_lookup + embedding_update_with_push_keys) bit for bit.  And run_wdl.train_laia with
cache_planned=True against False at world size 1."""
import os
import sys

import numpy as np
import pytest
import torch

from herald_amd import cache as hcache, hetu_ops
from herald_amd.sharded import ShardedEmbedding

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _own_tables(monkeypatch):
    # (the communicate op registers its store under the parameter's node id: keep those registrations out of later tests'
    # caches, which name node ids of their own)
    monkeypatch.setattr(hcache, "_TABLES", {})

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _ScriptedLoader:
    """(ids, sorted non-empty push plan) per batch, one set of device tensors per batch: get_arr / get_next_arr / peek_arr as
    LAIADataloader's."""

    def __init__(self, dev, nb, bs, rows, seed):
        rng = np.random.default_rng(seed)
        self.batches = []
        for _ in range(nb):
            ids = (np.minimum(rng.zipf(1.3, size=(bs, 26)) - 1, rows - 1) * 7919 % rows).astype(np.float32)
            u = np.unique(ids)
            plan = np.sort(rng.choice(u, size=max(1, u.size // 3), replace=False)).astype(np.float32)
            if rng.integers(0, 3) == 0:         # and keys of no line of the batch
                plan = np.unique(np.concatenate([plan, rng.integers(0, rows, size=5).astype(np.float32)]))
            self.batches.append((torch.from_numpy(ids).to(dev), torch.from_numpy(plan).to(dev)))
        self.k = 0

    def get_arr(self):
        b = self.batches[self.k]
        self.k += 1
        return b

    def get_next_arr(self):
        return self.batches[self.k] if self.k < len(self.batches) else None

    def peek_arr(self, j):
        i = self.k + j
        return self.batches[i] if i < len(self.batches) else None


def _run(dev, policy, planned, monkeypatch, nb=14):
    rows, width, bs, lr, limit, bound = 3000, 16, 8, 0.1, 300 if policy == "lru" else 120, 1
    rng = np.random.default_rng(5)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    store = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table0.copy()).to(dev))
    emb = hetu_ops.EmbeddingParameter(store=store)
    dl = _ScriptedLoader(dev, nb, bs, rows, 9)
    cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=True, cstable_policy=policy.upper(), cache_bound=bound,
                          cache_limit=limit, cache_plan_ahead=planned)
    comm = hetu_ops.ParameterServerCommunicateOp(emb, lr, dl.get_next_arr, peek_ids=dl.peek_arr if planned else None)
    comm.forward_hook(cfg)
    assert (comm._planned is not None) == planned
    if planned:
        def refuse(*a, **k):
            raise AssertionError("the planned run must not update call by call")
        monkeypatch.setattr(comm.cache.cache, "embedding_update_with_push_keys", refuse)
    look = hetu_ops.EmbeddingLookUp(emb, enable_push_index=True)
    look.forward_hook(cfg)
    gradop = hetu_ops.EmbeddingLookUp_Gradient(emb.shape, enable_push_index=True)
    pulled, scaled = [], []
    for k in range(nb - 1):
        ids_plan = dl.get_arr()
        out = torch.empty((bs, 26, width), dtype=torch.float32, device=dev)
        look.compute(ids_plan, out)
        pulled.append(out.clone())
        gout = (out * 0.25 - 0.5).contiguous()
        grad = gradop.compute(gout, ids_plan)
        assert grad.push_indices is ids_plan[1]
        comm.compute(grad)
        scaled.append(grad.values.clone())
    torch.cuda.synchronize()
    if planned:
        assert comm.cache.cache.plan_pending() > 0
    # the last batch pulled: its push alone (no next pull), so that both caches end on a finished pair
    ids_plan = dl.get_arr()
    out = torch.empty((bs, 26, width), dtype=torch.float32, device=dev)
    look.compute(ids_plan, out)
    pulled.append(out.clone())
    grad = gradop.compute((out * 0.25 - 0.5).contiguous(), ids_plan)
    comm._mult_lr(grad)
    comm._push(grad)
    torch.cuda.synchronize()
    comm.cache.cache.state()            # (raises when a bookkeeping launch left its sticky word)
    if planned:
        assert comm.cache.cache.plan_pending() == 0
    return pulled, scaled, store.table.clone(), comm.cache.cache._store[1].clone(), comm


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_comm_op_planned_push_plans_equal_call_by_call(dev, policy, monkeypatch):
    p_pull, p_scaled, p_table, p_ver, p_comm = _run(dev, policy, True, monkeypatch)
    c_pull, c_scaled, c_table, c_ver, c_comm = _run(dev, policy, False, monkeypatch)
    for k, (a, b) in enumerate(zip(p_pull, c_pull)):
        assert torch.equal(a, b), "pulled rows of step %d" % k
    for k, (a, b) in enumerate(zip(p_scaled, c_scaled)):
        assert torch.equal(a, b), "scaled gradients of step %d" % k
    assert torch.equal(p_table, c_table) and torch.equal(p_ver, c_ver)
    assert int(c_ver.sum()) > 0
    la, lb = p_comm.cache.cache.lines(), c_comm.cache.cache.lines()
    assert sorted(la) == sorted(lb)
    for key in la:
        assert (la[key].version, la[key].updates) == (lb[key].version, lb[key].updates), key
        np.testing.assert_array_equal(la[key].data, lb[key].data)
        np.testing.assert_array_equal(la[key].grad, lb[key].grad)


def test_comm_op_refuses_a_push_plan_it_was_not_planned_with(dev):
    rows, width, bs = 3000, 16, 8
    store = ShardedEmbedding(rows, width, dev, table=torch.zeros((rows, width), device=dev))
    emb = hetu_ops.EmbeddingParameter(store=store)
    dl = _ScriptedLoader(dev, 6, bs, rows, 3)
    cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=True, cstable_policy="LRU", cache_bound=1, cache_limit=300,
                          cache_plan_ahead=True)
    comm = hetu_ops.ParameterServerCommunicateOp(emb, 0.1, dl.get_next_arr, peek_ids=dl.peek_arr)
    comm.forward_hook(cfg)
    gradop = hetu_ops.EmbeddingLookUp_Gradient(emb.shape, enable_push_index=True)
    ids, plan = dl.get_arr()
    vals = torch.ones((bs, 26, width), device=dev)
    before = comm.cache.cache.plan_pending()
    for bad in ((ids, plan.clone()), ids, (ids.clone(), plan)):
        with pytest.raises(RuntimeError):
            comm.compute(gradop.compute(vals.clone(), bad) if isinstance(bad, tuple) else
                         hetu_ops.EmbeddingLookUp_Gradient(emb.shape).compute(vals.clone(), bad))
        assert comm.cache.cache.plan_pending() == before
    comm.compute(gradop.compute(vals.clone(), (ids, plan)))
    torch.cuda.synchronize()


def test_run_wdl_laia_cache_planned_equals_call_by_call(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))
    import run_wdl
    g = torch.Generator(device=dev).manual_seed(4)
    rows, width = 20000, 16
    table_init = torch.randn((rows, width), generator=g, device=dev) * 0.01
    runs = {}
    for planned in (False, True):
        losses, param, tower, comm = run_wdl.train_laia("wdl", rows, width, 32, 12, 0.05, cache="LRU", bound=0,
                                                        cache_limit=2000, device=str(dev), table_init=table_init,
                                                        cache_planned=planned)
        comm.cache.cache.state()        # (raises when a bookkeeping launch left its sticky word)
        runs[planned] = (losses, param.store.table.clone(), comm)
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1])
    assert runs[True][2]._planned is not None and runs[False][2]._planned is None
    assert runs[True][2].cache.cache.plan_pending() > 0
