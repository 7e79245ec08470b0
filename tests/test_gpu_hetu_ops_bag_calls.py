"""ParameterServerCommunicateOp(bag=F) with Config.cache_fuse_bag_calls on the schedules whose cache flow is call by call: bsp 0
without plan-ahead (embedding_lookup_sum + embedding_update_bags), LFU at bsp -1 (embedding_push_pull_bags) and laia (ids, push
plan) tuples with push_indices (embedding_update_with_push_keys_bags).  sparse_pull_val is [B, width], no gradient is expanded,
and the pooled rows of every step and the store equal the cache_fuse_bag_calls=False run bit for bit.  And the example:
run_wdl.train(model="emb_sum_wdl", embedding="cache") with and without the flag, LRU and LFU, gives equal losses and tables."""
import os
import sys

import numpy as np
import pytest
import torch

from herald_amd import cache as hcache, hetu_ops, ops
from herald_amd.sharded import ShardedEmbedding
from test_gpu_hetu_ops import _batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

F = 26
POOLED = ("embedding_lookup_sum", "embedding_update_bags", "embedding_update_with_push_keys_bags", "embedding_push_pull_bags")
UNPOOLED = ("embedding_lookup", "embedding_update", "embedding_update_with_push_keys", "embedding_push_pull")


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)
    import gc
    gc.collect()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


def _loop(dev, policy, bsp, laia, fuse, monkeypatch, nb=8):
    rows, width, bs, lr, limit, bound = 3000, 16, 8, 0.1, 8 * F + 40, 1
    rng = np.random.default_rng(2)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    store = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table0.copy()).to(dev))
    emb = hetu_ops.EmbeddingParameter(store=store)
    batches = _batches(nb, bs, rows, 9)
    ring = [torch.from_numpy(b).to(dev) for b in batches]
    if laia:        # (ids, push plan): every other unique key of the batch, ascending
        ring = [(t, torch.from_numpy(np.unique(b)[::2].astype(np.float32)).to(dev)) for t, b in zip(ring, batches)]
    state = {"k": 0}
    cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=bsp, prefetch=True, cstable_policy=policy.upper(), cache_bound=bound,
                          cache_limit=limit, cache_fuse_bag_calls=fuse)
    comm = hetu_ops.ParameterServerCommunicateOp(emb, lr, lambda: ring[(state["k"] + 1) % nb], bag=F)
    calls = {k: 0 for k in POOLED + UNPOOLED + ("expanded",)}
    orig_exp = ops.IndexedSlices.expanded_values
    monkeypatch.setattr(ops.IndexedSlices, "expanded_values",
                        lambda self, *a, **kw: (calls.__setitem__("expanded", calls["expanded"] + 1), orig_exp(self, *a, **kw))[1])
    for name in POOLED + UNPOOLED:
        orig = getattr(hcache._CacheBase, name)
        monkeypatch.setattr(hcache._CacheBase, name,
                            lambda self, *a, _o=orig, _k=name, **kw: (calls.__setitem__(_k, calls[_k] + 1), _o(self, *a, **kw))[1])
    comm.forward_hook(cfg, first_ids=ring[0])
    assert comm._planned is None and comm._bag_calls == fuse
    assert (comm._bag == F) if fuse else (comm._bag is None)
    assert tuple(comm.sparse_pull_val.shape) == ((bs, width) if fuse else (bs, F, width))
    assert (cfg.ps_pooled.get(emb) == F) if fuse else (emb not in cfg.ps_pooled)
    look = hetu_ops.EmbeddingLookUpSum(emb)
    look.forward_hook(cfg)
    gradop = hetu_ops.EmbeddingLookUpSum_Gradient(emb.shape, enable_push_index=laia)
    outs = []
    steps = nb - 1
    for k in range(steps):
        state["k"] = k
        ids = ring[k][0] if laia else ring[k]
        out = torch.empty((bs, width), dtype=torch.float32, device=dev)
        look.compute(ids, out)
        torch.cuda.synchronize()
        outs.append(_bits(out))
        gout = (out * 0.25 - 0.5).contiguous()
        comm.compute(gradop.compute(gout, ring[k]))
        torch.cuda.synchronize()
    pulls = "embedding_push_pull" if bsp < 0 else ("embedding_update_with_push_keys" if laia else "embedding_update")
    want = {k: 0 for k in calls}
    if fuse:       # nothing unpooled, nothing expanded (the first pull is made by forward_hook)
        want["embedding_lookup_sum"] = 1 if bsp < 0 else steps + 1
        want[pulls + "_bags"] = steps
    else:
        want["embedding_lookup"] = 1 if bsp < 0 else steps + 1
        want[pulls] = steps
        want["expanded"] = steps
    assert calls == want
    monkeypatch.undo()
    return comm, ring, outs, store.table.clone()


@pytest.mark.parametrize("policy,bsp,laia", [("lru", 0, False), ("lfu", -1, False), ("lfuopt", -1, False), ("lru", 0, True),
                                             ("lfu", 0, True)])
def test_call_by_call_flows_run_pooled_and_equal_the_unfused_run(dev, policy, bsp, laia, monkeypatch):
    _, _, outs_f, table_f = _loop(dev, policy, bsp, laia, True, monkeypatch)
    _, _, outs_u, table_u = _loop(dev, policy, bsp, laia, False, monkeypatch)
    assert len(outs_f) == len(outs_u) and all(np.array_equal(a, b) for a, b in zip(outs_f, outs_u))
    assert torch.equal(table_f.view(torch.int32), table_u.view(torch.int32))
    assert not np.array_equal(outs_f[0], outs_f[-1])


@pytest.mark.parametrize("bsp", [0, -1])
def test_pooled_calls_refuse_gradients_that_are_not_this_bags_pooled_slices(dev, bsp, monkeypatch):
    comm, ring, _, table = _loop(dev, "lfu", bsp, False, True, monkeypatch, nb=4)
    per_occ = hetu_ops.EmbeddingLookUp_Gradient(comm.parameter.shape).compute(
        torch.zeros((8, F, 16), dtype=torch.float32, device=dev), ring[3])
    other_bag = hetu_ops.EmbeddingLookUpSum_Gradient(comm.parameter.shape).compute(
        torch.zeros((16, 16), dtype=torch.float32, device=dev), ring[3].reshape(16, 13))
    for grad in (per_occ, other_bag):
        with pytest.raises(RuntimeError, match="the pull buffer holds pooled rows, so the gradients must be the pooled slices"):
            comm.compute(grad)
    torch.cuda.synchronize()
    assert torch.equal(comm.parameter.store.table, table)


@pytest.mark.parametrize("policy,bsp", [("LRU", 0), ("LFU", -1)])
def test_example_emb_sum_wdl_with_and_without_the_flag(dev, policy, bsp, monkeypatch):
    import run_wdl
    comms = []
    hook = hetu_ops.ParameterServerCommunicateOp.forward_hook
    monkeypatch.setattr(hetu_ops.ParameterServerCommunicateOp, "forward_hook",
                        lambda self, *a, **kw: (comms.append(self), hook(self, *a, **kw))[1])
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((20000, 16), generator=g, device=dev) * 0.01
    runs = {}
    for fuse in (True, False):
        losses, param, _ = run_wdl.train("cache", 20000, 16, 32, 8, 0.05, cache=policy, bound=2, table_init=table_init,
                                         device=str(dev), model="emb_sum_wdl", bsp=bsp, cache_fuse_bag_calls=fuse)
        torch.cuda.synchronize()
        comm = comms.pop()
        assert comm._bag_calls == fuse
        assert tuple(comm.sparse_pull_val.shape) == ((32, 16) if fuse else (32, run_wdl.NFIELD, 16))
        runs[fuse] = (losses, param.store.table.clone())
        del comm
    assert runs[True][0] == runs[False][0], "losses, step by step"
    assert torch.equal(runs[True][1].view(torch.int32), runs[False][1].view(torch.int32)), "the store's table"
    assert not torch.equal(runs[True][1], table_init)
