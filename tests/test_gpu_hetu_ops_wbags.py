"""EmbeddingLookUpWeightedSum + EmbeddingLookUpWeightedSum_Gradient (the embedding path of the FAE models): on a device table
the pair equals the ops calls bit for bit, fixed and ragged bags, and sgd_update_sparse applies the weighted slices fused; every
other consumer -- the other optimizers, the communicate op's push -- gives, bit for bit, what it gives on hand-expanded unpooled
slices; the forward out of a row buffer (the PS path) equals the device-table forward on equal rows."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wbag_model  # noqa: E402

from herald_amd import cache as hcache, hetu_ops, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR = 3000, 36, 9, 26, 0.05
OFFSETS = [0, 0, 30, 31, 100, 100, 234]        # ragged bags over the same B * F = 234 ids, empty ones among them


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module created and only the cyclic collector frees (operators that hold their configs, stores, plans) is
    collected here, with the device idle -- not at some later allocation inside another module's gated or timed call, where a
    finalizer that frees device memory would wait for that module's stream."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


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
    """Table, ids, weights and pooled gradients: built once, never written."""
    if not _shared:
        rng = np.random.default_rng(17)
        table = (rng.standard_normal((ROWS, WIDTH)) * np.exp(rng.uniform(-3, 3, (ROWS, 1)))).astype(np.float32)
        ids = rng.integers(1, ROWS, (B, F)).astype(np.float32)
        ids[:, 0] = 0                           # the padding id, dead, in every bag
        ids[:, 1] = 11                          # a live key in every bag: a run of B occurrences
        ids[2, 3] = ids[2, 7]                   # a key twice in one bag
        w = rng.standard_normal((B, F)).astype(np.float32)
        w[rng.random((B, F)) < 0.4] = 0
        w[:, 0] = 0
        w[:, 1] = 1
        w[4, 5] = np.float32(-0.0)
        _shared.update(table=table, ids=ids, w=w, g=rng.standard_normal((B, WIDTH)).astype(np.float32),
                       g_r=rng.standard_normal((len(OFFSETS) - 1, WIDTH)).astype(np.float32))
    return _shared


def _hbm(dev):
    param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(_inputs()["table"]).to(dev))
    return param, hetu_ops.Config(comm_mode=None, prefetch=False, use_sparse_pull=False)


def _layout(dev, ragged):
    """(ids, weights, offsets, bags, pooled gradient) on the device."""
    inp = _inputs()
    if ragged:
        return (torch.from_numpy(inp["ids"].reshape(-1)).to(dev), torch.from_numpy(inp["w"].reshape(-1)).to(dev),
                torch.tensor(OFFSETS, dtype=torch.int64, device=dev), len(OFFSETS) - 1, torch.from_numpy(inp["g_r"]).to(dev))
    return torch.from_numpy(inp["ids"]).to(dev), torch.from_numpy(inp["w"]).to(dev), None, B, torch.from_numpy(inp["g"]).to(dev)


def _weighted_slices(dev, ragged=False):
    d_ids, d_w, d_off, nb, d_g = _layout(dev, ragged)
    return hetu_ops.EmbeddingLookUpWeightedSum_Gradient((ROWS, WIDTH)).compute(d_g, d_ids, d_w, offsets=d_off)


def _hand_expanded(dev, ragged=False):
    """Ordinary unpooled slices with values = ops.wbag_grad_rows: what every consumer without a weighted form must see."""
    d_ids, d_w, d_off, nb, d_g = _layout(dev, ragged)
    if ragged:
        values = ops.wbag_grad_rows(d_g, d_w, bag_of=ops.bag_of(d_off, d_ids.numel()))
    else:
        values = ops.wbag_grad_rows(d_g, d_w.reshape(-1), bag=F)
    return ops.IndexedSlices(indices=d_ids, values=values, dense_shape=(ROWS, WIDTH))


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_the_operator_pair_on_a_device_table_equals_the_ops_calls(dev, ragged):
    inp = _inputs()
    d_ids, d_w, d_off, nb, d_g = _layout(dev, ragged)
    param, cfg = _hbm(dev)
    look = hetu_ops.EmbeddingLookUpWeightedSum(param)
    look.forward_hook(cfg)
    out = torch.full((nb, WIDTH), -1.0, dtype=torch.float32, device=dev)
    assert look.compute(d_ids, d_w, out, offsets=d_off) is out
    assert _same(out, ops.embedding_lookup_wsum(param.table, d_ids, d_w, offsets=d_off))
    off = np.array(OFFSETS, dtype=np.int64) if ragged else None
    ids = inp["ids"].reshape(-1) if ragged else inp["ids"]
    w = inp["w"].reshape(-1) if ragged else inp["w"]
    assert _same(out, torch.from_numpy(wbag_model.wbag_sum(inp["table"], ids, w, off)).to(dev))
    grad = hetu_ops.EmbeddingLookUpWeightedSum_Gradient(param.shape).compute(d_g, d_ids, d_w, offsets=d_off)
    assert grad.weighted and grad.pooled and not grad.fm_pooled and grad.values is d_g and grad.weights is d_w
    assert grad.indices is d_ids and tuple(grad.dense_shape) == (ROWS, WIDTH) and grad.push_indices is None
    assert (grad.bag == F and grad.bag_of is None) if not ragged else (grad.bag is None and grad.bag_of.numel() == B * F)
    hetu_ops.sgd_update_sparse(param, grad, LR)
    table2 = torch.from_numpy(inp["table"]).to(dev)
    ops.sgd_sparse_update_wbags(table2, d_ids, d_g, d_w, LR, offsets=d_off)
    assert _same(param.table, table2)
    g = inp["g_r"] if ragged else inp["g"]
    assert _same(param.table, torch.from_numpy(wbag_model.wbag_sgd(inp["table"], ids, w, g, LR, off)).to(dev))
    assert not _same(param.table, torch.from_numpy(inp["table"]).to(dev))
    assert _same(param.table[0], torch.from_numpy(inp["table"][0]).to(dev))        # the padding row: dead occurrences only
    # expanded_values and deduplicate go through ops.wbag_grad_rows
    assert _same(grad.expanded_values(), _hand_expanded(dev, ragged).values)
    a, b = _weighted_slices(dev, ragged).deduplicate(), _hand_expanded(dev, ragged).deduplicate()
    assert not a.weighted and not a.pooled and _same(a.indices, b.indices) and _same(a.values, b.values)


@pytest.mark.parametrize("fuse", [True, False], ids=["fuse_bags", "reference_sequence"])
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_adam_and_momentum_on_weighted_slices_equal_the_hand_expanded_call(dev, ragged, fuse):
    results = []
    for make in (_weighted_slices, _hand_expanded):
        param, _ = _hbm(dev)
        st1, st2, vel = torch.zeros_like(param.table), torch.zeros_like(param.table), torch.zeros_like(param.table)
        hetu_ops.adam_update_sparse(param, make(dev, ragged), st1, st2, LR, 0.9, 0.999, 0.9, 0.999, 1e-7, fuse_bags=fuse)
        mparam, _ = _hbm(dev)
        hetu_ops.momentum_update_sparse(mparam, make(dev, ragged), vel, LR, 0.9, False, fuse_bags=fuse)
        results.append((param.table, st1, st2, mparam.table, vel))
    for a, b in zip(*results):
        assert _same(a, b)
    start = torch.from_numpy(_inputs()["table"]).to(dev)
    assert not _same(results[0][0], start) and not _same(results[0][3], start)


def _ps_step(dev, grad, d_ids):
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(_inputs()["table"].copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids)
    comm.forward_hook(hetu_ops.Config(comm_mode="PS", prefetch=False), first_ids=d_ids)
    comm.compute(grad)
    torch.cuda.synchronize()
    return store.table


def test_a_communicate_op_step_on_the_sharded_store_equals_the_hand_expanded_step(dev):
    d_ids = _layout(dev, False)[0]
    grad = _weighted_slices(dev)
    got = _ps_step(dev, grad, d_ids)
    want = _ps_step(dev, _hand_expanded(dev), d_ids)
    assert _same(got, want)
    assert not _same(got, torch.from_numpy(_inputs()["table"]).to(dev))
    # the learning rate went into the expanded values: the caller's pooled gradient and weights are as they were
    assert grad.weighted and _same(grad.values, torch.from_numpy(_inputs()["g"]).to(dev))


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_the_forward_from_a_row_buffer_equals_the_device_table_forward(dev, ragged):
    d_ids, d_w, d_off, nb, _ = _layout(dev, ragged)
    param, cfg = _hbm(dev)
    want = ops.embedding_lookup_wsum(param.table, d_ids, d_w, offsets=d_off)
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(_inputs()["table"].copy()).to(dev))
    ps_param = hetu_ops.EmbeddingParameter(store=store)
    look = hetu_ops.EmbeddingLookUpWeightedSum(ps_param)
    look.forward_hook(hetu_ops.Config(comm_mode="PS", prefetch=False))
    out = torch.full((nb, WIDTH), -1.0, dtype=torch.float32, device=dev)
    look.compute(d_ids, d_w, out, offsets=d_off)
    torch.cuda.synchronize()
    assert _same(out, want)


def test_a_pooled_pull_buffer_is_refused(dev):
    """A communicate op that pulls POOLED rows (bag=) holds unweighted sums: the weighted lookup cannot be served from them."""
    d_ids, d_w, _, nb, _ = _layout(dev, False)
    store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(_inputs()["table"].copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    cfg = hetu_ops.Config(comm_mode="PS", prefetch=True)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids, bag=F)
    comm.forward_hook(cfg, first_ids=d_ids)
    assert cfg.ps_pooled.get(param) == F
    look = hetu_ops.EmbeddingLookUpWeightedSum(param)
    look.forward_hook(cfg)
    with pytest.raises(ValueError, match="pooled rows"):
        look.compute(d_ids, d_w, torch.empty((nb, WIDTH), dtype=torch.float32, device=dev))
