"""EmbeddingLookUpFM + EmbeddingLookUpFM_Gradient (the second-order term of the DeepFM models) on three tiers: a device table
(the fused kernel), a world-1 sharded store behind ParameterServerCommunicateOp, and an LRU cache with bound 0 in front of that
store, call by call.  The rows, the sum and the FM output are bit-equal across the tiers and equal tests/fm_model.py; after one
update the table equals the model's -- the serial per-occurrence SGD on the device table; the scaled, per-key reduced push on
the store; and for the cache both: its lines take the scaled gradients occurrence by occurrence (oracle/cache_model.py,
Line.accumulate: data + v_i0 + v_i1 ..., which is the serial SGD's row - lr*g_i0 - lr*g_i1 ... bit for bit) and stay current
after the push at bound 0, so a lookup through the cache returns the serial model's rows while the store behind it holds the
reduced push."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_model  # noqa: E402

from herald_amd import cache as hcache, hetu_ops, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR = 3000, 36, 9, 26, 0.05


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    """A communicate op with a cache registers its store under the parameter's node id (cache.register_table), process-wide:
    leave the registry as it was, so that later modules' caches with the same node ids find no table of ours."""
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_shared = {}


def _inputs():
    """Table, ids, the two gradients and the model's outputs: built once, shared by every tier, never written."""
    if not _shared:
        rng = np.random.default_rng(5)
        table = (rng.standard_normal((ROWS, WIDTH)) * np.exp(rng.uniform(-4, 4, (ROWS, 1)))).astype(np.float32)
        ids = rng.integers(0, ROWS, (B, F)).astype(np.float32)
        ids[:, 0] = 11                          # a key in every bag: a run of B occurrences
        ids[2, 3] = ids[2, 7]                   # a key twice in one bag
        g = rng.standard_normal((B, F, WIDTH)).astype(np.float32)
        gf = rng.standard_normal((B, WIDTH)).astype(np.float32)
        rows, covered, S, fm = fm_model.fm_lookup(table, ids)
        grad = fm_model.fm_grad_rows(g, rows, S, gf, bag=F)
        _shared.update(table=table, ids=ids, g=g, gf=gf, rows=rows, S=S, fm=fm, grad=grad,
                       serial=fm_model.sgd_serial(table, ids, grad, LR), pushed=fm_model.ps_push(table, ids, grad, LR))
    return _shared


def _run(dev, tier):
    """One forward, one backward, one update on a tier; returns (rows, sum, fm, gradient values, the table after -- read through
    a lookup for the cache --, the store's own table or None)."""
    inp = _inputs()
    d_ids = torch.from_numpy(inp["ids"]).to(dev)
    comm = None
    if tier == "hbm":
        param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(inp["table"]).to(dev))
        cfg = hetu_ops.Config(comm_mode=None, prefetch=False, use_sparse_pull=False)
    else:
        store = ShardedEmbedding(ROWS, WIDTH, dev, table=torch.from_numpy(inp["table"].copy()).to(dev))
        param = hetu_ops.EmbeddingParameter(store=store)
        if tier == "ps":
            cfg = hetu_ops.Config(comm_mode="PS", prefetch=False)
        else:
            cfg = hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=False, cstable_policy="LRU", cache_bound=0,
                                  cache_limit=1000)
        comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids)
        comm.forward_hook(cfg, first_ids=d_ids)
    look = hetu_ops.EmbeddingLookUpFM(param)
    look.forward_hook(cfg)
    assert look._fused == (tier == "hbm")
    rows = torch.full((B, F, WIDTH), -1.0, dtype=torch.float32, device=dev)
    S = torch.full((B, WIDTH), -1.0, dtype=torch.float32, device=dev)
    fm = torch.full((B, WIDTH), -1.0, dtype=torch.float32, device=dev)
    got = look.compute(d_ids, rows, S, fm)
    assert got[0] is rows and got[1] is S and got[2] is fm
    torch.cuda.synchronize()
    outs = (_bits(rows), _bits(S), _bits(fm))
    vectors = torch.from_numpy(inp["g"]).to(dev)
    grad = hetu_ops.EmbeddingLookUpFM_Gradient(param.shape).compute(vectors, torch.from_numpy(inp["gf"]).to(dev), rows, S, d_ids)
    assert not grad.pooled and grad.values.data_ptr() == vectors.data_ptr() and grad.push_indices is None
    assert grad.indices is d_ids and tuple(grad.dense_shape) == (ROWS, WIDTH)
    values = _bits(grad.values)
    store_table = None
    if tier == "hbm":
        hetu_ops.sgd_update_sparse(param, grad, LR)
        torch.cuda.synchronize()
        table = param.table.cpu().numpy()
    else:
        comm.compute(grad)                   # -lr scale, push
        torch.cuda.synchronize()
        store_table = param.store.table.cpu().numpy()
        table = store_table.copy()
        if tier == "cache":                  # the rows the batch touched are read through the cache, which holds their lines
            touched = np.unique(inp["ids"])
            dest = torch.empty((touched.size, WIDTH), dtype=torch.float32, device=dev)
            param.cache.embedding_lookup(torch.from_numpy(touched).to(dev), dest).wait()
            table[touched.astype(np.int64)] = dest.cpu().numpy()
    return outs + (values, table, store_table)


@pytest.fixture(scope="module")
def runs(dev):
    return {tier: _run(dev, tier) for tier in ("hbm", "ps", "cache")}


def test_outputs_equal_the_model_and_are_bit_equal_across_the_tiers(runs):
    inp = _inputs()
    for tier, (rows, S, fm, values, _, _) in runs.items():
        assert np.array_equal(rows.reshape(-1, WIDTH), _bits(inp["rows"])), tier
        assert np.array_equal(S, _bits(inp["S"])), tier
        assert np.array_equal(fm, _bits(inp["fm"])), tier
        assert np.array_equal(values.reshape(-1, WIDTH), _bits(inp["grad"])), tier
    for tier in ("ps", "cache"):
        for a, b in zip(runs["hbm"][:4], runs[tier][:4]):
            assert np.array_equal(a, b), tier


def test_table_after_one_update_equals_the_models(runs):
    inp = _inputs()
    assert np.array_equal(_bits(runs["hbm"][4]), _bits(inp["serial"]))
    assert np.array_equal(_bits(runs["ps"][4]), _bits(inp["pushed"]))
    assert np.array_equal(_bits(runs["cache"][4]), _bits(inp["serial"]))         # through the cache: its lines
    assert np.array_equal(_bits(runs["cache"][5]), _bits(inp["pushed"]))         # behind it: the store
    assert not np.array_equal(_bits(inp["serial"]), _bits(inp["pushed"]))        # (duplicate keys: the two orders differ)
    assert not np.array_equal(_bits(inp["serial"]), _bits(inp["table"]))
    touched = np.unique(inp["ids"].astype(np.int64))
    assert np.all(np.any(inp["pushed"][touched] != inp["table"][touched], axis=1))


def test_gradient_operator_ragged_bags_push_indices_and_no_row_gradient(dev):
    inp = _inputs()
    n = B * F
    off = np.array([0, 0, 30, 31, 200, n], dtype=np.int64)
    flat = inp["ids"].reshape(-1)
    d_flat, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)
    param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(inp["table"]).to(dev))
    look = hetu_ops.EmbeddingLookUpFM(param)
    look.forward_hook(hetu_ops.Config(comm_mode=None, prefetch=False, use_sparse_pull=False))
    nb = off.size - 1
    rows = torch.empty((n, WIDTH), dtype=torch.float32, device=dev)
    S = torch.empty((nb, WIDTH), dtype=torch.float32, device=dev)
    fm = torch.empty((nb, WIDTH), dtype=torch.float32, device=dev)
    look.compute(d_flat, rows, S, fm, offsets=d_off)
    rows_m, covered, S_m, fm_m = fm_model.fm_lookup(inp["table"], flat, off)
    assert covered.all()
    assert np.array_equal(_bits(rows), _bits(rows_m)) and np.array_equal(_bits(S), _bits(S_m))
    assert np.array_equal(_bits(fm), _bits(fm_m))
    gf = inp["gf"][:nb]
    plan_keys = torch.from_numpy(np.unique(flat)[::2].copy()).to(dev)
    gradop = hetu_ops.EmbeddingLookUpFM_Gradient(param.shape, enable_push_index=True)
    grad = gradop.compute(None, torch.from_numpy(gf.copy()).to(dev), rows, S, (d_flat, plan_keys), offsets=d_off)
    assert grad.push_indices is plan_keys and grad.indices is d_flat and not grad.pooled
    assert np.array_equal(_bits(grad.values), _bits(fm_model.fm_grad_rows(None, rows_m, S_m, gf, offsets=off)))
    with pytest.raises(TypeError):
        gradop.compute(None, torch.from_numpy(gf.copy()).to(dev), rows, S, d_flat, offsets=d_off)
    with pytest.raises(ValueError):
        hetu_ops.EmbeddingLookUpFM_Gradient(param.shape).compute(None, torch.from_numpy(gf.copy()).to(dev), rows, S, d_flat)
