"""examples/ctr/run_wdl.py --model fae_wdl --embedding ps --ps-fuse-wbags: the cold table of the FAE Wide & Deep behind the sharded
store, as the reference keeps it on ctx=ht.cpu(0).  The communicate op gets the cold ids and the cold mask of batch k + 1 and
bag=26, pulls weighted pooled rows (store.pull_wsum) and pushes the weighted pooled slices as they are (push_wbags).  The run is
compared, bit for bit in losses, table, hot table and tower, with a run of the same example whose communicate op is built without
next_weights (and without bag=): per-occurrence rows, the weighted summing pass, the expanded gradient."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR = 2000, 16, 16, 4, 0.05


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """As tests/test_gpu_example_fae_wdl.py: what only the cyclic collector frees is collected here, with the device idle."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


def _train(dev, bsp):
    import run_wdl
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    losses, param, tower = run_wdl.train("ps", ROWS, WIDTH, BATCH, STEPS, LR, table_init=table_init, device=str(dev),
                                         model="fae_wdl", bsp=bsp, fae_hot_rate=0.05, ps_fuse_wbags=True)
    torch.cuda.synchronize()
    return losses, param, tower, table_init


@pytest.mark.parametrize("bsp", [0, -1])
def test_fae_wdl_on_the_ps_tier_equals_the_expanded_path(dev, bsp, monkeypatch):
    import run_wdl
    from herald_amd import hetu_ops
    from herald_amd.sharded import ShardedEmbedding
    calls = {"pull_wsum": 0, "push_wbags": 0, "pull": 0, "push": 0}
    for name in calls:
        def spy(self, *a, _orig=getattr(ShardedEmbedding, name), _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(ShardedEmbedding, name, spy)
    losses, param, tower, table_init = _train(dev, bsp)
    assert calls == {"pull_wsum": STEPS + 1, "push_wbags": STEPS, "pull": 0, "push": 0}
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
    for name in calls:
        calls[name] = 0
    losses2, param2, tower2, _ = _train(dev, bsp)
    assert calls == {"pull_wsum": 0, "push_wbags": 0, "pull": STEPS + 1, "push": STEPS}
    assert losses == losses2
    assert np.array_equal(_bits(param.store.table), _bits(param2.store.table))
    assert np.array_equal(_bits(param.hot_table), _bits(param2.hot_table))
    for a, b in zip(tower.parameters(), tower2.parameters()):
        assert np.array_equal(_bits(a), _bits(b))


def test_without_the_flag_the_refusal_stands_and_names_the_flag(dev):
    import run_wdl
    with pytest.raises(ValueError, match="fae_wdl.*ps-fuse-wbags"):
        run_wdl.train("ps", ROWS, WIDTH, BATCH, 2, LR, device=str(dev), model="fae_wdl")
    for embedding in ("cache", "step", "step3", "queue"):
        with pytest.raises(ValueError, match="fae_wdl"):
            run_wdl.train(embedding, ROWS, WIDTH, BATCH, 2, LR, device=str(dev), model="fae_wdl", ps_fuse_wbags=True)
    with pytest.raises(ValueError, match="fae_deepfm"):
        run_wdl.train("ps", ROWS, WIDTH, BATCH, 2, LR, device=str(dev), model="fae_deepfm", ps_fuse_wbags=True)
