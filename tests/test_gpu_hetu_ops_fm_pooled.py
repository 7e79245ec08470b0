"""EmbeddingLookUpFMSum + EmbeddingLookUpFMSum_Gradient (the second-order term of the pooled DeepFM) on a device table: the
lookup gives embedding_lookup_fm's sum and FM output bit for bit and writes no rows; the gradient operator returns FM-pooled
IndexedSlices, and sgd_update_sparse on them equals, bit for bit, the composed operators -- EmbeddingLookUpFM,
EmbeddingLookUpFM_Gradient with the expanded g_sum as `vectors`, sgd_update_sparse.  Every other consumer of slices refuses
FM-pooled ones, and the lookup refuses every tier but the device table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_model  # noqa: E402
import fm_pooled_model  # noqa: E402

from herald_amd import cache as hcache, hetu_ops, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR = 3000, 36, 9, 26, 0.05
OFFSETS = [0, 0, 30, 31, 100, 100, 234]        # ragged bags over the same B * F = 234 ids, empty ones among them


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    """A communicate op with a cache registers its store process-wide (cache.register_table): leave the registry as it was."""
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_shared = {}


def _inputs():
    """Table, ids and the gradients of S and of the FM output: built once, never written."""
    if not _shared:
        rng = np.random.default_rng(7)
        table = (rng.standard_normal((ROWS, WIDTH)) * np.exp(rng.uniform(-3, 3, (ROWS, 1)))).astype(np.float32)
        ids = rng.integers(0, ROWS, (B, F)).astype(np.float32)
        ids[:, 0] = 11                          # a key in every bag: a run of B occurrences
        ids[2, 3] = ids[2, 7]                   # a key twice in one bag
        _shared.update(table=table, ids=ids, gs=rng.standard_normal((B, WIDTH)).astype(np.float32),
                       gf=rng.standard_normal((B, WIDTH)).astype(np.float32),
                       gs_r=rng.standard_normal((len(OFFSETS) - 1, WIDTH)).astype(np.float32),
                       gf_r=rng.standard_normal((len(OFFSETS) - 1, WIDTH)).astype(np.float32))
    return _shared


def _hbm(dev):
    param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(_inputs()["table"]).to(dev))
    return param, hetu_ops.Config(comm_mode=None, prefetch=False, use_sparse_pull=False)


def _layout(dev, ragged):
    inp = _inputs()
    if ragged:
        return (torch.from_numpy(inp["ids"].reshape(-1)).to(dev), torch.tensor(OFFSETS, dtype=torch.int64, device=dev),
                len(OFFSETS) - 1, inp["gs_r"], inp["gf_r"])
    return torch.from_numpy(inp["ids"]).to(dev), None, B, inp["gs"], inp["gf"]


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_lookup_gives_the_fm_lookups_sum_and_fm(dev, ragged):
    d_ids, d_off, nb, _, _ = _layout(dev, ragged)
    param, cfg = _hbm(dev)
    look = hetu_ops.EmbeddingLookUpFMSum(param)
    look.forward_hook(cfg)
    S = torch.full((nb, WIDTH), -1.0, dtype=torch.float32, device=dev)
    fm = torch.full((nb, WIDTH), -1.0, dtype=torch.float32, device=dev)
    got = look.compute(d_ids, S, fm, offsets=d_off)
    assert got[0] is S and got[1] is fm
    _, S_ref, fm_ref = ops.embedding_lookup_fm(param.table, d_ids, offsets=d_off)
    assert _same(S, S_ref) and _same(fm, fm_ref)
    assert _same(param.table, torch.from_numpy(_inputs()["table"]).to(dev))


@pytest.mark.parametrize("with_sum", [True, False], ids=["g_sum", "no_g_sum"])
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_gradient_and_sgd_equal_the_composed_operators(dev, ragged, with_sum):
    inp = _inputs()
    d_ids, d_off, nb, gs, gf = _layout(dev, ragged)
    d_gs = torch.from_numpy(gs).to(dev) if with_sum else None
    d_gf = torch.from_numpy(gf).to(dev)
    # the pooled pair
    param, cfg = _hbm(dev)
    look = hetu_ops.EmbeddingLookUpFMSum(param)
    look.forward_hook(cfg)
    S = torch.empty((nb, WIDTH), dtype=torch.float32, device=dev)
    fm = torch.empty((nb, WIDTH), dtype=torch.float32, device=dev)
    look.compute(d_ids, S, fm, offsets=d_off)
    grad = hetu_ops.EmbeddingLookUpFMSum_Gradient(param.shape).compute(d_gs, d_gf, S, d_ids, offsets=d_off)
    assert grad.fm_pooled and grad.pooled and grad.values is d_gs and grad.fm_grad is d_gf and grad.fm_sum is S
    assert grad.indices is d_ids and tuple(grad.dense_shape) == (ROWS, WIDTH) and grad.push_indices is None
    assert (grad.bag == F and grad.bag_of is None) if not ragged else (grad.bag is None and grad.bag_of.numel() == B * F)
    hetu_ops.sgd_update_sparse(param, grad, LR)
    # the composed operators
    param2, cfg2 = _hbm(dev)
    look2 = hetu_ops.EmbeddingLookUpFM(param2)
    look2.forward_hook(cfg2)
    rows2 = torch.empty(tuple(d_ids.shape) + (WIDTH,), dtype=torch.float32, device=dev)
    S2 = torch.empty((nb, WIDTH), dtype=torch.float32, device=dev)
    fm2 = torch.empty((nb, WIDTH), dtype=torch.float32, device=dev)
    look2.compute(d_ids, rows2, S2, fm2, offsets=d_off)
    assert _same(S, S2) and _same(fm, fm2)
    vectors = None
    if with_sum:
        which = torch.arange(B * F, device=dev) // F if not ragged else ops.bag_of(d_off, B * F).long()
        vectors = d_gs[which].reshape(tuple(d_ids.shape) + (WIDTH,)).contiguous()
    grad2 = hetu_ops.EmbeddingLookUpFM_Gradient(param2.shape).compute(vectors, d_gf, rows2, S2, d_ids, offsets=d_off)
    assert not grad2.pooled
    hetu_ops.sgd_update_sparse(param2, grad2, LR)
    assert _same(param.table, param2.table)
    # ... and the restatement
    off = np.array(OFFSETS, dtype=np.int64) if ragged else None
    ids = inp["ids"].reshape(-1) if ragged else inp["ids"]
    _, _, S_m, _ = fm_model.fm_lookup(inp["table"], ids, off)
    want = fm_pooled_model.fm_pooled_sgd(inp["table"], ids, gs if with_sum else None, gf, S_m, LR, off)
    assert _same(param.table, torch.from_numpy(want).to(dev))
    assert not _same(param.table, torch.from_numpy(inp["table"]).to(dev))


def _fm_pooled_slices(dev):
    inp = _inputs()
    d_ids = torch.from_numpy(inp["ids"]).to(dev)
    S = torch.from_numpy(inp["gs"]).to(dev)
    return hetu_ops.EmbeddingLookUpFMSum_Gradient((ROWS, WIDTH)).compute(torch.from_numpy(inp["gs"]).to(dev),
                                                                       torch.from_numpy(inp["gf"]).to(dev), S, d_ids), d_ids


def test_the_other_optimizers_refuse_fm_pooled_slices(dev):
    grad, _ = _fm_pooled_slices(dev)
    param, _ = _hbm(dev)
    before = param.table.clone()
    st1, st2 = torch.zeros_like(param.table), torch.zeros_like(param.table)
    for fuse in (True, False):
        with pytest.raises(ValueError, match="FM-pooled"):
            hetu_ops.momentum_update_sparse(param, grad, st1, LR, 0.9, False, fuse_bags=fuse)
        with pytest.raises(ValueError, match="FM-pooled"):
            hetu_ops.adagrad_update_sparse(param, grad, st1, LR, 1e-7, fuse_bags=fuse)
        with pytest.raises(ValueError, match="FM-pooled"):
            hetu_ops.adam_update_sparse(param, grad, st1, st2, LR, 0.9, 0.999, 0.9, 0.999, 1e-7, fuse_bags=fuse)
        with pytest.raises(ValueError, match="FM-pooled"):
            hetu_ops.adamw_update_sparse(param, grad, st1, st2, LR, 0.9, 0.999, 0.9, 0.999, 1e-7, 0.01, fuse_bags=fuse)
    assert _same(param.table, before) and not st1.any() and not st2.any()


def test_the_communicate_op_refuses_fm_pooled_slices(dev):
    grad, d_ids = _fm_pooled_slices(dev)
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(_inputs()["table"].copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids)
    comm.forward_hook(hetu_ops.Config(comm_mode="PS", prefetch=False), first_ids=d_ids)
    before = store.table.clone()
    with pytest.raises(ValueError, match="FM-pooled"):
        comm.compute(grad)
    torch.cuda.synchronize()
    assert _same(store.table, before)


@pytest.mark.parametrize("tier", ["ps", "ps_prefetch", "cache"])
def test_forward_hook_refuses_every_tier_but_the_device_table(dev, tier):
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(_inputs()["table"].copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = {"ps": hetu_ops.Config(comm_mode="PS", prefetch=False),
           "ps_prefetch": hetu_ops.Config(comm_mode="PS", prefetch=True),
           "cache": hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=False, cstable_policy="LRU", cache_bound=0,
                                    cache_limit=1000)}[tier]
    with pytest.raises(ValueError, match="device table"):
        hetu_ops.EmbeddingLookUpFMSum(param).forward_hook(cfg)
