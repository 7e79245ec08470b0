"""ParameterServerCommunicateOp(bag=F) in the asp-with-prefetch schedule (bsp < 0, prefetch) with Config.cache_plan_ahead, peek_ids
and Config.cache_fuse_bags: the head, every step and the last pull are ONE pooled cache call each through the planned push-pull
chain (embedding_push_pull_planned_bags); sparse_pull_val is [B, width], no gradient is expanded.  The pooled rows equal
bag_model.bag_sum over the rows of oracle/cache_model.py and the server table equals the model's, every step, bit for bit.
With cache_fuse_bags off, and with LFU (call by call at bsp < 0), nothing is pooled and the same values come out.  And the example:
run_wdl.train at bsp -1 with fusion on equals the run with fusion off, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import bag_model
from herald_amd import hetu_ops, ops
from herald_amd.sharded import ShardedEmbedding
from oracle import cache_model, cpu
from test_gpu_hetu_ops import _batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

F = 26


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    from herald_amd import cache as hcache
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)
    import gc
    gc.collect()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _loop(dev, policy, fuse, monkeypatch, nb=12, run_dry=False):
    rows, width, bs, lr, limit, bound = 3000, 16, 8, 0.1, 2 * 8 * F + 40, 1
    rng = np.random.default_rng(2)
    table0 = rng.standard_normal((rows, width), dtype=np.float32)
    store = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table0.copy()).to(dev))
    emb = hetu_ops.EmbeddingParameter(store=store)
    batches = _batches(nb, bs, rows, 9)
    state = {"k": 0}
    ring = [torch.from_numpy(b).to(dev) for b in batches]

    def next_ids():
        return ring[(state["k"] + 1) % len(batches)]

    def peek_ids(j):
        i = state["k"] + 1 + j
        if run_dry and j > 0 and i % 3 == 0:          # the loader sometimes knows only the very next batch
            return None
        return ring[i] if i < len(batches) else None

    cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=-1, prefetch=True, cstable_policy=policy.upper(), cache_bound=bound,
                          cache_limit=limit, cache_plan_ahead=True, cache_fuse_bags=fuse)
    comm = hetu_ops.ParameterServerCommunicateOp(emb, lr, next_ids, peek_ids=peek_ids, bag=F)
    calls = {"pooled": 0, "unpooled": 0, "expanded": 0}
    orig_exp = ops.IndexedSlices.expanded_values
    monkeypatch.setattr(ops.IndexedSlices, "expanded_values",
                        lambda self, *a, **kw: (calls.__setitem__("expanded", calls["expanded"] + 1), orig_exp(self, *a, **kw))[1])
    comm.forward_hook(cfg, first_ids=ring[0])
    pooled = fuse and policy == "lru"
    assert comm._chain == (policy == "lru")
    assert (comm._bag == F) if pooled else (comm._bag is None)
    assert tuple(comm.sparse_pull_val.shape) == ((bs, width) if pooled else (bs, F, width))
    raw = comm.cache.cache
    for name, key in (("embedding_push_pull_planned_bags", "pooled"), ("embedding_push_pull_planned", "unpooled")):
        orig = getattr(raw, name)
        setattr(raw, name, lambda *a, _o=orig, _k=key, **kw: (calls.__setitem__(_k, calls[_k] + 1), _o(*a, **kw))[1])
    look = hetu_ops.EmbeddingLookUpSum(emb)
    look.forward_hook(cfg)
    gradop = hetu_ops.EmbeddingLookUpSum_Gradient(emb.shape)
    server = cache_model.Server(table0)
    model = cache_model.CacheModel(policy, limit, width, server, bound, bound)
    pending = model.lookup(batches[0].reshape(-1).astype(np.uint64))
    pos = np.arange(bs * F).reshape(bs, F)
    outs = []
    for k in range(len(batches) - 1):
        state["k"] = k
        ids, d_ids = batches[k], ring[k]
        out = torch.empty((bs, width), dtype=torch.float32, device=dev)
        look.compute(d_ids, out)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(bag_model.bag_sum(pending.reshape(bs * F, width), pos)),
                                      err_msg="pooled lookup step %d" % k)
        outs.append(_bits(out))
        gout = (out * 0.25 - 0.5).contiguous()
        g_np = cpu.scale_values(gout.cpu().numpy(), lr)                       # [bs, width] * -lr: the same product per occurrence
        comm.compute(gradop.compute(gout, d_ids))
        pending = model.push_pull(batches[k + 1].reshape(-1).astype(np.uint64), ids.reshape(-1).astype(np.uint64),
                                  np.ascontiguousarray(g_np[np.arange(bs * F) // F]))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(store.table.cpu().numpy(), server.table, err_msg="server table step %d" % k)
    steps = len(batches) - 1
    if pooled:
        # ONE pooled cache call per step (and the head, made by forward_hook before the counters were in place); nothing expanded
        assert calls == {"pooled": steps, "unpooled": 0, "expanded": 0}
    elif policy == "lru":
        assert calls == {"pooled": 0, "unpooled": steps, "expanded": steps}
    else:
        assert calls["pooled"] == 0 and calls["unpooled"] == 0 and calls["expanded"] == steps
    return comm, ring, outs, store.table.clone()


@pytest.mark.parametrize("run_dry", [False, True])
def test_asp_prefetch_pooled_goes_through_the_pooled_chain(dev, run_dry, monkeypatch):
    _loop(dev, "lru", True, monkeypatch, run_dry=run_dry)


def test_asp_pooled_chain_equals_the_unfused_chain_and_lfu_stays_unfused(dev, monkeypatch):
    _, _, outs_f, table_f = _loop(dev, "lru", True, monkeypatch)
    _, _, outs_u, table_u = _loop(dev, "lru", False, monkeypatch)
    assert all(np.array_equal(a, b) for a, b in zip(outs_f, outs_u))
    assert torch.equal(table_f.view(torch.int32), table_u.view(torch.int32))
    _loop(dev, "lfu", True, monkeypatch)               # LFU at bsp < 0: call by call, per-occurrence rows, the model's values


def test_asp_pooled_chain_refuses_per_occurrence_gradients(dev, monkeypatch):
    comm, ring, _, _ = _loop(dev, "lru", True, monkeypatch, nb=4)
    gradop = hetu_ops.EmbeddingLookUp_Gradient(comm.parameter.shape)
    grad = gradop.compute(torch.zeros((8, F, 16), dtype=torch.float32, device=dev), ring[3])
    pending = comm.cache.cache.plan_pending()
    with pytest.raises(RuntimeError, match="pooled"):
        comm.compute(grad)
    assert comm.cache.cache.plan_pending() == pending


@pytest.mark.parametrize("fuse", [True, False])
def test_example_emb_sum_wdl_asp_planned(dev, fuse, monkeypatch):
    """The example at the command line's default schedule: the communicate op's buffer and bag size with and without fusion,
    and a table that training has changed (tests/test_gpu_example_emb_sum_asp_planned_bags.py compares the two runs)."""
    import run_wdl
    comms = []
    hook = hetu_ops.ParameterServerCommunicateOp.forward_hook
    monkeypatch.setattr(hetu_ops.ParameterServerCommunicateOp, "forward_hook",
                        lambda self, *a, **kw: (comms.append(self), hook(self, *a, **kw))[1])
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((20000, 16), generator=g, device=dev) * 0.01
    losses, param, _ = run_wdl.train("cache", 20000, 16, 32, 8, 0.05, cache="LRU", bound=2, table_init=table_init,
                                     device=str(dev), model="emb_sum_wdl", bsp=-1, cache_planned=True, cache_fuse_bags=fuse)
    torch.cuda.synchronize()
    comm = comms.pop()
    assert tuple(comm.sparse_pull_val.shape) == ((32, 16) if fuse else (32, run_wdl.NFIELD, 16))
    assert (comm._bag == run_wdl.NFIELD) if fuse else (comm._bag is None)
    assert len(losses) == 8 and all(np.isfinite(losses))
    assert not torch.equal(param.store.table, table_init)
    del comm
