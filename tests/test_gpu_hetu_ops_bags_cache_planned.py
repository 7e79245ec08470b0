"""examples/ctr/run_wdl.py --model emb_sum_wdl --embedding cache --cache-planned --bsp 0: the communicate op is told the bag
size and, with Config.cache_fuse_bags (the default), pulls POOLED rows (embedding_lookup_sum_planned) and pushes the pooled
gradient as it is (embedding_update_planned_bags).  Held to the same run with cache_fuse_bags off -- per-occurrence rows, a
summing pass, the expanded gradient --, which it equals bit for bit: the loss of every step and the store's table."""
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
    leave the registry as it was, so that later modules' caches with the same node ids find no table of ours."""
    from herald_amd import cache as hcache
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)
    # a communicate op keeps bound methods of itself (compute, _push, _pull): it, its cache and the cache's device memory go
    # with the cycle collector only -- here, not at some allocation in the middle of a later module's training run
    import gc
    gc.collect()


@pytest.mark.parametrize("policy", ["LRU", "LFU"])
def test_pooled_planned_pairs_equal_the_unfused_path_bit_for_bit(dev, policy, monkeypatch):
    import run_wdl
    from herald_amd import hetu_ops
    comms = []          # the communicate op of the run under way (train() keeps it to itself)
    hook = hetu_ops.ParameterServerCommunicateOp.forward_hook

    def recording_hook(self, *a, **kw):
        comms.append(self)
        return hook(self, *a, **kw)

    monkeypatch.setattr(hetu_ops.ParameterServerCommunicateOp, "forward_hook", recording_hook)
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    runs = {}
    for fuse in (True, False):
        losses, param, _ = run_wdl.train("cache", ROWS, WIDTH, BATCH, STEPS, LR, cache=policy, bound=2, table_init=table_init,
                                         device=str(dev), model="emb_sum_wdl", bsp=0, cache_planned=True, cache_fuse_bags=fuse)
        torch.cuda.synchronize()
        comm = comms.pop()
        assert not comms and comm.parameter is param
        # with fusion on the communicate op never asks for an [n, width] tensor: its pull buffer is the pooled one
        assert tuple(comm.sparse_pull_val.shape) == ((BATCH, WIDTH) if fuse else (BATCH, run_wdl.NFIELD, WIDTH))
        assert (comm._bag == run_wdl.NFIELD) if fuse else (comm._bag is None)
        runs[fuse] = (losses, param.store.table.clone())
        del comm
    assert runs[True][0] == runs[False][0], "losses, step by step"
    assert torch.equal(runs[True][1].view(torch.int32), runs[False][1].view(torch.int32)), "the store's table"
    assert not torch.equal(runs[True][1], table_init)          # the table must have changed
