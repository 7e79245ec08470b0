"""examples/ctr/run_wdl.py --model fae_wdl --embedding cache --cache {lfu,lru} --bound 0 --cache-planned --bsp 0
--cache-fuse-wbags: the cold table of the FAE Wide & Deep behind the HET cache, the configuration of the reference's
examples/ctr/tests/hybrid_fae_wdl_criteo.sh.  The communicate op gets the cold ids and the cold mask of batch k + 1 and bag=26,
pulls weighted pooled rows (embedding_lookup_wsum_planned) and pushes the weighted pooled slices as they are
(embedding_update_planned_wbags).  The run is compared, bit for bit in losses, table, hot table and tower, with a run of the same
example whose communicate op is built without next_weights (and without bag=): per-occurrence planned pairs, the weighted
summing pass, the expanded gradient."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR = 4000, 16, 32, 6, 0.05


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    from herald_amd import cache as hcache
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


def _train(dev, policy):
    import run_wdl
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    losses, param, tower = run_wdl.train("cache", ROWS, WIDTH, BATCH, STEPS, LR, cache=policy, bound=0, table_init=table_init,
                                         device=str(dev), model="fae_wdl", bsp=0, cache_planned=True, cache_fuse_wbags=True,
                                         fae_hot_rate=0.05)
    torch.cuda.synchronize()
    return losses, param, tower, table_init


@pytest.mark.parametrize("policy", ["lfu", "lru"])
def test_fae_wdl_on_the_cache_tier_equals_the_expanded_path(dev, policy, monkeypatch):
    import run_wdl
    from herald_amd import cache as hcache
    from herald_amd import hetu_ops
    names = ("embedding_lookup_wsum_planned", "embedding_update_planned_wbags", "embedding_lookup_planned",
             "embedding_update_planned")
    calls = dict.fromkeys(names, 0)
    for name in names:
        def spy(self, *a, _orig=getattr(hcache.CacheSparseTable, name), _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(hcache.CacheSparseTable, name, spy)
    losses, param, tower, table_init = _train(dev, policy)
    assert calls == {"embedding_lookup_wsum_planned": STEPS + 1, "embedding_update_planned_wbags": STEPS,
                     "embedding_lookup_planned": 0, "embedding_update_planned": 0}
    assert len(losses) == STEPS and all(np.isfinite(losses))
    assert not np.array_equal(_bits(param.store.table), _bits(table_init))
    assert param.hot_table.shape[0] == int(0.05 * ROWS)

    # the same example with the op built without next_weights (and bag=): the expanded path
    orig = hetu_ops.ParameterServerCommunicateOp

    def expanded_op(parameter, learning_rate, next_ids, peek_ids=None, bag=None, next_weights=None):
        return orig(parameter, learning_rate, next_ids, peek_ids=peek_ids)

    def expanded_hook(self, config, first_ids=None, barrier=lambda: None, first_weights=None, _hook=orig.forward_hook):
        return _hook(self, config, first_ids=first_ids, barrier=barrier)

    monkeypatch.setattr(run_wdl.hetu_ops, "ParameterServerCommunicateOp", expanded_op)
    monkeypatch.setattr(orig, "forward_hook", expanded_hook)
    for name in names:
        calls[name] = 0
    losses2, param2, tower2, _ = _train(dev, policy)
    assert calls == {"embedding_lookup_wsum_planned": 0, "embedding_update_planned_wbags": 0,
                     "embedding_lookup_planned": STEPS + 1, "embedding_update_planned": STEPS}
    assert losses == losses2
    assert np.array_equal(_bits(param.store.table), _bits(param2.store.table))
    assert np.array_equal(_bits(param.hot_table), _bits(param2.hot_table))
    for a, b in zip(tower.parameters(), tower2.parameters()):
        assert np.array_equal(_bits(a), _bits(b))


def test_every_other_fae_wdl_run_on_the_cache_is_refused(dev):
    import run_wdl
    kw = dict(device=str(dev), model="fae_wdl")
    for extra in (dict(), dict(cache_planned=True, bsp=0), dict(cache_fuse_wbags=True, bsp=0),
                  dict(cache_fuse_wbags=True, cache_planned=True, bsp=-1)):
        with pytest.raises(ValueError, match="fae_wdl"):
            run_wdl.train("cache", ROWS, WIDTH, BATCH, 2, LR, **kw, **extra)
