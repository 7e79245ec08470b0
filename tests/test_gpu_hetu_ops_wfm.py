"""EmbeddingLookUpWeightedFMSum + EmbeddingLookUpWeightedFMSum_Gradient (the second-order term of the FAE DeepFM): on a device
table the pair plus sgd_update_sparse equals the ops calls bit for bit, fixed and ragged bags; every other consumer -- the PS and
cache tiers, the other optimizers, the communicate op's push, unweighted_slices -- refuses the slices and changes nothing."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wfm_model  # noqa: E402

from herald_amd import hetu_ops, ops  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, WIDTH, B, F, LR = 3000, 36, 9, 26, 0.05
OFFSETS = [0, 0, 30, 31, 100, 100, 234]        # ragged bags over the same B * F = 234 ids, empty ones among them


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module created and only the cyclic collector frees (operators that hold their configs, stores, plans) is
    collected here, with the device idle."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


class _Store:
    """What EmbeddingParameter and the refusals read of a store.  Every refusal below comes before the store is used, so this
    module builds no sharded store, no cache and no communicate flow: it creates no stream, and the modules that run after it
    find the streams they would have found without it."""

    def __init__(self, table):
        self.table, self.rows, self.width, self.world = table, table.shape[0], table.shape[1], 1


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_shared = {}


def _inputs():
    """Table, ids, weights and the two pooled gradients: built once, never written."""
    if not _shared:
        rng = np.random.default_rng(18)
        table = (rng.standard_normal((ROWS, WIDTH)) * np.exp(rng.uniform(-3, 3, (ROWS, 1)))).astype(np.float32)
        ids = rng.integers(1, ROWS, (B, F)).astype(np.float32)
        ids[:, 0] = 0                           # the padding id, dead, in every bag
        ids[:, 1] = 11                          # a live key in every bag: a run of B occurrences
        ids[2, 3] = ids[2, 7]                   # a key twice in one bag
        ids[3, 9] = ROWS + 4                    # an id beyond the table, its weight not zero
        w = rng.standard_normal((B, F)).astype(np.float32)
        w[rng.random((B, F)) < 0.4] = 0
        w[:, 0] = 0
        w[:, 1] = 1
        w[3, 9] = 2
        w[4, 5] = np.float32(-0.0)
        nr = len(OFFSETS) - 1
        _shared.update(table=table, ids=ids, w=w, gs=rng.standard_normal((B, WIDTH)).astype(np.float32),
                       gq=rng.standard_normal((B, WIDTH)).astype(np.float32),
                       gs_r=rng.standard_normal((nr, WIDTH)).astype(np.float32),
                       gq_r=rng.standard_normal((nr, WIDTH)).astype(np.float32))
    return _shared


def _hbm(dev):
    param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(_inputs()["table"]).to(dev))
    return param, hetu_ops.Config(comm_mode=None, prefetch=False, use_sparse_pull=False)


def _layout(dev, ragged):
    """(ids, weights, offsets, bags, g_S, g_Q) on the device."""
    inp = _inputs()
    if ragged:
        return (torch.from_numpy(inp["ids"].reshape(-1)).to(dev), torch.from_numpy(inp["w"].reshape(-1)).to(dev),
                torch.tensor(OFFSETS, dtype=torch.int64, device=dev), len(OFFSETS) - 1, torch.from_numpy(inp["gs_r"]).to(dev),
                torch.from_numpy(inp["gq_r"]).to(dev))
    return (torch.from_numpy(inp["ids"]).to(dev), torch.from_numpy(inp["w"]).to(dev), None, B, torch.from_numpy(inp["gs"]).to(dev),
            torch.from_numpy(inp["gq"]).to(dev))


def _slices(dev, ragged=False):
    d_ids, d_w, d_off, nb, d_gs, d_gq = _layout(dev, ragged)
    grad = hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient((ROWS, WIDTH)).compute(d_gs, d_gq, d_ids, d_w, offsets=d_off)
    return grad, d_ids


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_the_operator_pair_on_a_device_table_equals_the_ops_calls(dev, ragged):
    inp = _inputs()
    d_ids, d_w, d_off, nb, d_gs, d_gq = _layout(dev, ragged)
    param, cfg = _hbm(dev)
    look = hetu_ops.EmbeddingLookUpWeightedFMSum(param)
    look.forward_hook(cfg)
    S = torch.full((nb, WIDTH), -1.0, dtype=torch.float32, device=dev)
    Q = torch.full((nb, WIDTH), -1.0, dtype=torch.float32, device=dev)
    got = look.compute(d_ids, d_w, S, Q, offsets=d_off)
    assert got[0] is S and got[1] is Q
    want_S, want_Q = ops.embedding_lookup_wfm(param.table, d_ids, d_w, offsets=d_off)
    assert _same(S, want_S) and _same(Q, want_Q)
    off = np.array(OFFSETS, dtype=np.int64) if ragged else None
    ids = inp["ids"].reshape(-1) if ragged else inp["ids"]
    w = inp["w"].reshape(-1) if ragged else inp["w"]
    m_S, m_Q = wfm_model.wfm_lookup(inp["table"], ids, w, off)
    assert _same(S, torch.from_numpy(m_S).to(dev)) and _same(Q, torch.from_numpy(m_Q).to(dev))
    grad = hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient(param.shape).compute(d_gs, d_gq, d_ids, d_w, offsets=d_off)
    assert grad.weighted_fm and grad.weighted and grad.pooled and not grad.fm_pooled
    assert grad.values is d_gs and grad.sq_grad is d_gq and grad.weights is d_w
    assert grad.indices is d_ids and tuple(grad.dense_shape) == (ROWS, WIDTH) and grad.push_indices is None
    assert (grad.bag == F and grad.bag_of is None) if not ragged else (grad.bag is None and grad.bag_of.numel() == B * F)
    hetu_ops.sgd_update_sparse(param, grad, LR)
    table2 = torch.from_numpy(inp["table"]).to(dev)
    ops.sgd_sparse_update_wfm_bags(table2, d_ids, d_gs, d_gq, d_w, LR, offsets=d_off)
    assert _same(param.table, table2)
    gs, gq = (inp["gs_r"], inp["gq_r"]) if ragged else (inp["gs"], inp["gq"])
    assert _same(param.table, torch.from_numpy(wfm_model.wfm_sgd(inp["table"], ids, w, gs, gq, LR, off)).to(dev))
    assert not _same(param.table, torch.from_numpy(inp["table"]).to(dev))
    assert _same(param.table[0], torch.from_numpy(inp["table"][0]).to(dev))        # the padding row: dead occurrences only
    # the weighted branch alone would have dropped the Q term
    table3 = torch.from_numpy(inp["table"]).to(dev)
    ops.sgd_sparse_update_wbags(table3, d_ids, d_gs, d_w, LR, offsets=d_off)
    assert not _same(param.table, table3)


def test_push_indices_are_refused(dev):
    d_ids, d_w, _, _, d_gs, d_gq = _layout(dev, False)
    with pytest.raises(TypeError):
        hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient((ROWS, WIDTH)).compute(d_gs, d_gq, (d_ids, d_ids), d_w)
    with pytest.raises(ValueError):
        hetu_ops.EmbeddingLookUpWeightedFMSum_Gradient((ROWS, WIDTH)).compute(d_gs, d_gq, d_ids.reshape(-1), d_w.reshape(-1))


@pytest.mark.parametrize("tier", ["ps", "ps_prefetch", "cache"])
def test_forward_hook_refuses_every_tier_but_the_device_table(dev, tier):
    param = hetu_ops.EmbeddingParameter(store=_Store(torch.from_numpy(_inputs()["table"].copy()).to(dev)))
    cfg = {"ps": hetu_ops.Config(comm_mode="PS", prefetch=False),
           "ps_prefetch": hetu_ops.Config(comm_mode="PS", prefetch=True),
           "cache": hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=False, cstable_policy="LRU", cache_bound=0,
                                    cache_limit=1000)}[tier]
    with pytest.raises(ValueError, match="device table"):
        hetu_ops.EmbeddingLookUpWeightedFMSum(param).forward_hook(cfg)


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_the_other_optimizers_and_unweighted_slices_refuse_the_slices(dev, ragged):
    grad, _ = _slices(dev, ragged)
    param, _ = _hbm(dev)
    before = param.table.clone()
    st1, st2 = torch.zeros_like(param.table), torch.zeros_like(param.table)
    for fuse in (True, False):
        with pytest.raises(ValueError, match="table row"):
            hetu_ops.momentum_update_sparse(param, grad, st1, LR, 0.9, False, fuse_bags=fuse)
        with pytest.raises(ValueError, match="table row"):
            hetu_ops.adagrad_update_sparse(param, grad, st1, LR, 1e-7, fuse_bags=fuse)
        with pytest.raises(ValueError, match="table row"):
            hetu_ops.adam_update_sparse(param, grad, st1, st2, LR, 0.9, 0.999, 0.9, 0.999, 1e-7, fuse_bags=fuse)
        with pytest.raises(ValueError, match="table row"):
            hetu_ops.adamw_update_sparse(param, grad, st1, st2, LR, 0.9, 0.999, 0.9, 0.999, 1e-7, 0.01, fuse_bags=fuse)
    with pytest.raises(ValueError, match="table row"):
        hetu_ops.unweighted_slices(grad)
    for call in (grad.expanded_values, grad.deduplicate, grad.to_dense):
        with pytest.raises(ValueError, match="table row"):
            call()
    assert _same(param.table, before) and not st1.any() and not st2.any()
    assert grad.weighted_fm


def test_the_communicate_op_refuses_the_slices(dev):
    grad, d_ids = _slices(dev)
    store = _Store(torch.from_numpy(_inputs()["table"].copy()).to(dev))
    param = hetu_ops.EmbeddingParameter(store=store)
    comm = hetu_ops.ParameterServerCommunicateOp(param, LR, next_ids=lambda: d_ids)
    before = store.table.clone()
    # every schedule's compute begins with _per_occurrence, the op's one door for slices: refused there, before any push
    for compute in (comm._compute_no_prefetch, comm._compute_bsp_prefetch, comm._compute_ssp_prefetch,
                    comm._compute_asp_prefetch):
        with pytest.raises(ValueError, match="weighted FM-pooled"):
            compute(grad)
    torch.cuda.synchronize()
    assert _same(store.table, before) and grad.weighted_fm
    # and sgd_update_sparse without a device table
    with pytest.raises(ValueError, match="device table"):
        hetu_ops.sgd_update_sparse(param, grad, LR)
