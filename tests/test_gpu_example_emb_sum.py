"""examples/ctr/run_wdl.py --model emb_sum_wdl (the reference's emb_sum_wdl_criteo: embedding_lookup_op followed by
reduce_sum_op(axes=1), a sample's 26 rows summed into one before the tower) against the same training loop in plain
PyTorch ops, with the table in HBM (the fused sum-pooled lookup and the bag apply), behind the PS and behind the cache.

PyTorch sums a bag in its own order and sums the gradients of duplicate ids before the update, so the runs agree within
rounding: the sizes and tolerances are those of tests/test_gpu_example_wdl.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))

pytestmark = pytest.mark.gpu

ROWS, WIDTH, BATCH, STEPS, LR = 30000, 16, 128, 12, 0.05
RTOL = 1e-5
ATOL = 5e-7


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    """A communicate op with a cache registers its store under the parameter's node id (cache.register_table), process-wide:
    leave the registry as it was, so that later modules' caches with the same node ids find no table of ours."""
    from herald_amd import cache as hcache
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)


def _torch_reference(dev, table_init):
    import run_wdl
    tower = run_wdl.make_tower("emb_sum_wdl", WIDTH, 0).to(dev)
    table = table_init.clone()
    opt = torch.optim.SGD(tower.parameters(), lr=LR)
    batches = run_wdl.make_batches(min(STEPS + 1, 64), BATCH, ROWS, 0)
    losses = []
    for k in range(STEPS):
        ids, dense, label = (torch.from_numpy(a).to(dev) for a in batches[k % len(batches)])
        idx = ids.long()
        emb = table[idx].clone().requires_grad_(True)
        pred = tower(dense, emb.sum(1))
        loss = torch.nn.functional.binary_cross_entropy(pred, label)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        table.index_add_(0, idx.reshape(-1), emb.grad.reshape(-1, WIDTH), alpha=-LR)
        losses.append(float(loss.detach()))
    return losses, table, tower


@pytest.fixture(scope="module")
def reference(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    table_init = torch.randn((ROWS, WIDTH), generator=g, device=dev) * 0.01
    return table_init, _torch_reference(dev, table_init)


@pytest.mark.parametrize("embedding,kw", [("hbm", {}), ("ps", {}), ("cache", {"cache": "LRU", "bound": 0})])
def test_emb_sum_wdl_training_matches_pytorch(dev, reference, embedding, kw):
    import run_wdl
    table_init, (ref_losses, ref_table, ref_tower) = reference
    losses, param, tower = run_wdl.train(embedding, ROWS, WIDTH, BATCH, STEPS, LR, table_init=table_init, device=str(dev),
                                         model="emb_sum_wdl", **kw)
    assert tower.W4.shape == (256 + WIDTH, 1)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    if embedding == "cache":
        # rows the cache still holds with unpushed updates are not in the store yet: compare through a lookup
        touched = torch.unique(torch.cat([torch.from_numpy(b[0]).reshape(-1) for b in
                                          run_wdl.make_batches(STEPS, BATCH, ROWS, 0)])).to(dev)
        dest = torch.empty((touched.numel(), WIDTH), dtype=torch.float32, device=dev)
        param.cache.embedding_lookup(touched, dest).wait()
        got, want, init = dest, ref_table[touched.long()], table_init[touched.long()]
    else:
        got = param.table if param.table is not None else param.store.table
        want, init = ref_table, table_init
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)
    for p, q in zip(tower.parameters(), ref_tower.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-7)
    assert not torch.equal(want, init)          # the table must have changed


@pytest.mark.parametrize("embedding", ["queue", "step", "step3"])
def test_step_engines_refuse_the_pooled_model(dev, embedding):
    import run_wdl
    with pytest.raises(ValueError, match="pools its embeddings"):
        run_wdl.train(embedding, 2000, 16, 8, 2, 0.05, device=str(dev), model="emb_sum_wdl")
