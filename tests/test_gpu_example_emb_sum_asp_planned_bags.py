"""examples/ctr/run_wdl.py --model emb_sum_wdl --embedding cache --cache lru --cache-planned at the default --bsp -1 (asp with
prefetch): every training step is ONE cache call through the planned push-pull chain, and with Config.cache_fuse_bags (the
default) that call is pooled on both sides (embedding_push_pull_planned_bags): the communicate op's pull buffer is
[batch, width] and the [batch, width] gradient is pushed as it is.  Held to the same run with cache_fuse_bags off -- the
unpooled chain: per-occurrence rows, a summing pass, the expanded gradient --, which it equals bit for bit: the loss of every
step and the store's table."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR = 20000, 16, 32, 8, 0.05


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    """A communicate op with a cache registers its store under the parameter's node id (cache.register_table), process-wide:
    leave the registry as it was, and let the op, its cache and the cache's device memory go here, with the cycle collector."""
    from herald_amd import cache as hcache
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)
    import gc
    gc.collect()


def test_pooled_asp_chain_equals_the_unfused_chain_bit_for_bit(dev, monkeypatch):
    import run_wdl
    from herald_amd import cache as hcache, hetu_ops
    comms = []          # the communicate op of the run under way (train() keeps it to itself)
    hook = hetu_ops.ParameterServerCommunicateOp.forward_hook

    def recording_hook(self, *a, **kw):
        comms.append(self)
        return hook(self, *a, **kw)

    monkeypatch.setattr(hetu_ops.ParameterServerCommunicateOp, "forward_hook", recording_hook)
    calls = {"pooled": 0, "unpooled": 0}
    for name, key in (("embedding_push_pull_planned_bags", "pooled"), ("embedding_push_pull_planned", "unpooled")):
        orig = getattr(hcache.CacheSparseTable, name)
        monkeypatch.setattr(hcache.CacheSparseTable, name,
                            lambda self, *a, _o=orig, _k=key, **kw: (calls.__setitem__(_k, calls[_k] + 1), _o(self, *a, **kw))[1])
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    runs = {}
    for fuse in (True, False):
        calls["pooled"] = calls["unpooled"] = 0
        losses, param, _ = run_wdl.train("cache", ROWS, WIDTH, BATCH, STEPS, LR, cache="LRU", bound=2, table_init=table_init,
                                         device=str(dev), model="emb_sum_wdl", bsp=-1, cache_planned=True, cache_fuse_bags=fuse)
        torch.cuda.synchronize()
        comm = comms.pop()
        assert not comms and comm.parameter is param and comm._chain
        # with fusion the communicate op never asks for an [n, width] tensor: its pull buffer is the pooled one
        assert tuple(comm.sparse_pull_val.shape) == ((BATCH, WIDTH) if fuse else (BATCH, run_wdl.NFIELD, WIDTH))
        assert (comm._bag == run_wdl.NFIELD) if fuse else (comm._bag is None)
        # the head and every step: ONE cache call each, pooled or not at all
        assert calls == ({"pooled": STEPS + 1, "unpooled": 0} if fuse else {"pooled": 0, "unpooled": STEPS})
        runs[fuse] = (losses, param.store.table.clone())
        del comm
    assert runs[True][0] == runs[False][0], "losses, step by step"
    assert torch.equal(runs[True][1].view(torch.int32), runs[False][1].view(torch.int32)), "the store's table"
    assert not torch.equal(runs[True][1], table_init)          # the table must have changed
