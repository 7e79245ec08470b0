"""Sum-pooled embedding lookup ("bags") and its sparse SGD apply on the GPU: ha_gather_sum_* against the numpy restatement
(tests/bag_model.py) bit for bit, ha_sgd_apply_bags against ha_sgd_apply on the expanded gradient and against
ha_apply_mapped with the same bag map, bit for bit, and the operator layer on top of them."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402

from herald_amd import _lib, hetu_ops, ops  # noqa: E402
from herald_amd.sharded import ShardedEmbedding  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 3000


@pytest.fixture(autouse=True)
def _table_registry_as_found():
    """A communicate op with a cache registers its store under the parameter's node id (cache.register_table), process-wide:
    leave the registry as it was, so that later modules' caches with the same node ids find no table of ours."""
    from herald_amd import cache as hcache
    before = dict(hcache._TABLES)
    yield
    hcache._TABLES.clear()
    hcache._TABLES.update(before)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_tables = {}


def _table(width):
    """One table per width, shared and never written: magnitudes over many binades so that the order of a sum shows, row 5
    all -0.0."""
    if width not in _tables:
        rng = np.random.default_rng(width)
        t = (rng.standard_normal((ROWS, width)) * np.exp(rng.uniform(-8, 8, (ROWS, 1)))).astype(np.float32)
        t[5] = -0.0
        _tables[width] = t
    return _tables[width]


def _device_chain(rows_bfd):
    """embedding_lookup's rows [B, F, d] summed by sequential float32 adds on the device."""
    acc = torch.zeros((rows_bfd.shape[0], rows_bfd.shape[2]), dtype=torch.float32, device=rows_bfd.device)
    for j in range(rows_bfd.shape[1]):
        acc = acc + rows_bfd[:, j]
    return acc


def _fixed_ids(B, F, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, ROWS, (B, F)).astype(np.float32)
    if F >= 2:
        ids[0, 1] = ids[0, 0]              # a duplicate id inside a bag
    ids[B - 1, F - 1] = ROWS + 3           # an id >= rows: a zero row
    ids[min(1, B - 1), 0] = 5              # the -0.0 row
    return ids


@pytest.mark.parametrize("F", [1, 2, 26, 27, 65])
@pytest.mark.parametrize("d", [1, 3, 4, 64, 68, 128, 512, 516])
def test_forward_fixed_bags_equal_the_restatement_bit_for_bit(dev, d, F):
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    for B in (1, 3, 257):
        ids = _fixed_ids(B, F, 100 * F + B)
        d_ids = torch.from_numpy(ids).to(dev)
        out = ops.embedding_lookup_sum(d_table, d_ids)
        assert out.shape == (B, d)
        want = bag_model.bag_sum(table, ids)
        assert np.array_equal(_bits(out), _bits(want)), (d, F, B)
        chain = _device_chain(ops.embedding_lookup(d_table, d_ids))
        assert np.array_equal(_bits(out), _bits(chain)), (d, F, B)


def test_forward_int64_ids_and_every_slice_width(dev):
    d, B, F = 512, 33, 26
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    ids = _fixed_ids(B, F, 7)
    want = _bits(bag_model.bag_sum(table, ids))
    d_ids64 = torch.from_numpy(ids.astype(np.int64)).to(dev)
    assert np.array_equal(_bits(ops.embedding_lookup_sum(d_table, d_ids64)), want)
    L = _lib.load()
    try:
        for floats in (64, 128, 256):              # results do not depend on how a bag's columns are cut into waves
            assert L.ha_debug_bag_slice(floats) == 0
            assert np.array_equal(_bits(ops.embedding_lookup_sum(d_table, d_ids64)), want), floats
            assert np.array_equal(_bits(ops.embedding_lookup_sum(d_table, torch.from_numpy(ids).to(dev))), want), floats
    finally:
        L.ha_debug_bag_slice(0)


def test_forward_minus_zero_row_in_a_bag_of_one_sums_to_plus_zero(dev):
    d_table = torch.from_numpy(_table(4)).to(dev)
    out = ops.embedding_lookup_sum(d_table, torch.tensor([[5.0]], device=dev))
    assert np.array_equal(_bits(out), np.zeros((1, 4), np.int32))


def test_forward_rows_beyond_2_to_24(dev):
    rows, d = (1 << 24) + 64, 4
    d_table = torch.zeros((rows, d), dtype=torch.float32, device=dev)
    top = np.array([(1 << 24) + 2, (1 << 24) + 62, (1 << 24) - 1, (1 << 24) + 4, 7, (1 << 24) + 62], dtype=np.int64)
    rng = np.random.default_rng(24)
    vals = (rng.standard_normal((rows - ((1 << 24) - 8), d)) * 100).astype(np.float32)
    d_table[(1 << 24) - 8:] = torch.from_numpy(vals).to(dev)
    d_table[7] = 3.25
    ids = top.astype(np.float32).reshape(3, 2)
    assert np.array_equal(ids.astype(np.int64).reshape(-1), top)       # (all exactly representable)
    out = ops.embedding_lookup_sum(d_table, torch.from_numpy(ids).to(dev))
    picked = d_table[torch.from_numpy(top).to(dev)].cpu().numpy()       # [6, d]
    want = bag_model.bag_sum(picked, np.arange(6, dtype=np.float32).reshape(3, 2))
    assert np.array_equal(_bits(out), _bits(want))
    assert np.abs(want).min() > 0


@pytest.mark.parametrize("d", [3, 64, 516])
def test_forward_ragged_bags(dev, d):
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    rng = np.random.default_rng(d)
    n = 1300
    ids = rng.integers(0, ROWS, n).astype(np.float32)
    ids[3], ids[700] = ROWS + 1, 5
    d_ids = torch.from_numpy(ids).to(dev)
    layouts = {
        "empty first, middle and last bag": [0, 0, 10, 37, 37, 37, 300, 1300, 1300],
        "one bag holding all ids": [0, 1300],
        "one bag of 1,000 ids": [0, 100, 1100, 1101, 1300],
    }
    for name, off in layouts.items():
        off = np.array(off, dtype=np.int64)
        B = off.size - 1
        # one guard row behind the output stays untouched
        buf = torch.full((B + 1, d), 12345.0, dtype=torch.float32, device=dev)
        out = ops.embedding_lookup_sum(d_table, d_ids, offsets=torch.from_numpy(off).to(dev), out=buf[:B])
        want = bag_model.bag_sum(table, ids, off)
        assert np.array_equal(_bits(out), _bits(want)), name
        assert torch.all(buf[B] == 12345.0), name
        assert np.array_equal(ops.bag_of(torch.from_numpy(off).to(dev), n).cpu().numpy(), bag_model.bag_of(off, n)), name
    # n = 0: every bag is empty
    off = torch.zeros(4, dtype=torch.int64, device=dev)
    out = ops.embedding_lookup_sum(d_table, torch.empty(0, dtype=torch.float32, device=dev), offsets=off)
    assert np.array_equal(_bits(out), np.zeros((3, d), np.int32))


def test_forward_ragged_offsets_are_clamped(dev):
    """Offsets that are not what the contract asks for read no id at or beyond n and write no row at or beyond B."""
    d, n = 8, 40
    table = _table(d)
    d_table = torch.from_numpy(table).to(dev)
    ids = np.arange(n).astype(np.float32)
    off = np.array([0, 50, 20, -3, 1 << 40], dtype=np.int64)
    buf = torch.full((5, d), 7.0, dtype=torch.float32, device=dev)
    out = ops.embedding_lookup_sum(d_table, torch.from_numpy(ids).to(dev), offsets=torch.from_numpy(off).to(dev), out=buf[:4])
    assert np.array_equal(_bits(out), _bits(bag_model.bag_sum(table, ids, off)))
    assert torch.all(buf[4] == 7.0)


# ---- backward ---------------------------------------------------------------------------------------------------------------
def _planted_ids(B, F, rows, seed):
    """Runs of 1-3, 4-47, 48+ and 300+ occurrences (the short, medium, long and tolerance-tree classes of the apply), a key
    twice in one bag included."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1000, rows, B * F)
    pos = rng.permutation(B * F)
    ids[pos[:20]] = 11                      # medium
    ids[pos[20:120]] = 12                   # long
    ids[pos[120:520]] = 13                  # the tolerance tree's class
    ids[pos[520:522]] = 14                  # short
    ids = ids.reshape(B, F)
    ids[0, :2] = 15                         # a key twice in one bag
    ids[1, 3] = ids[1, 7] = 12
    ids[2, 0] = rows + 9                    # out of range: ignored
    return ids.astype(np.float32)


@pytest.mark.parametrize("tolerance", [0, 1])
@pytest.mark.parametrize("d", [3, 64, 65, 128, 512])
def test_backward_fixed_bags_equal_the_expanded_apply_bit_for_bit(dev, d, tolerance):
    B, F, rows, lr = 64, 26, 5000, 0.05
    rng = np.random.default_rng(d)
    table0 = rng.standard_normal((rows, d)).astype(np.float32)
    ids = _planted_ids(B, F, rows, d)
    counts = np.unique(ids, return_counts=True)[1]
    assert counts.max() >= 300 and np.any((counts >= 48) & (counts < 300)) and np.any((counts >= 4) & (counts < 48)) and \
        np.any(counts <= 3)
    g = rng.standard_normal((B, d)).astype(np.float32)
    d_ids, d_g = torch.from_numpy(ids).to(dev), torch.from_numpy(g).to(dev)
    plan = ops.IndexPlan(B * F, dev).sort(d_ids.reshape(-1))
    prev = ops.set_tolerance_mode(tolerance)
    try:
        t_exp = torch.from_numpy(table0).to(dev)
        ops.sgd_apply(t_exp, plan, d_g.repeat_interleave(F, 0).contiguous(), lr)
        t_bag = torch.from_numpy(table0).to(dev)
        ops.sgd_apply_bags(t_bag, plan, d_g, lr, bag=F)
        t_one = torch.from_numpy(table0).to(dev)
        ops.sgd_sparse_update_bags(t_one, d_ids, d_g, lr)               # the one-call form
        t_one64 = torch.from_numpy(table0).to(dev)
        ops.sgd_sparse_update_bags(t_one64, d_ids.to(torch.int64), d_g, lr)
        torch.cuda.synchronize()
    finally:
        ops.set_tolerance_mode(prev)
    assert np.array_equal(_bits(t_bag), _bits(t_exp))
    assert np.array_equal(_bits(t_one), _bits(t_exp))
    assert np.array_equal(_bits(t_one64), _bits(t_exp))
    assert not np.array_equal(_bits(t_bag), _bits(table0))
    if not tolerance:
        assert np.array_equal(_bits(t_bag), _bits(bag_model.sgd_bags(table0, ids, g, lr)))


def test_backward_fixed_bags_beyond_the_small_plan(dev):
    """n = 36,868 crosses the plan's 36,864-id threshold."""
    B, F, d, rows, lr = 1418, 26, 4, 20000, 0.1
    rng = np.random.default_rng(3)
    table0 = rng.standard_normal((rows, d)).astype(np.float32)
    ids = rng.integers(0, rows, (B, F))
    ids[rng.random((B, F)) < 0.05] = 77
    ids = ids.astype(np.float32)
    g = rng.standard_normal((B, d)).astype(np.float32)
    d_ids, d_g = torch.from_numpy(ids).to(dev), torch.from_numpy(g).to(dev)
    plan = ops.IndexPlan(B * F, dev).sort(d_ids.reshape(-1))
    t_exp = torch.from_numpy(table0).to(dev)
    ops.sgd_apply(t_exp, plan, d_g.repeat_interleave(F, 0).contiguous(), lr)
    t_bag = torch.from_numpy(table0).to(dev)
    ops.sgd_apply_bags(t_bag, plan, d_g, lr, bag=F)
    t_one = torch.from_numpy(table0).to(dev)
    ops.sgd_sparse_update_bags(t_one, d_ids, d_g, lr)
    assert np.array_equal(_bits(t_bag), _bits(t_exp))
    assert np.array_equal(_bits(t_one), _bits(t_exp))
    assert not np.array_equal(_bits(t_bag), _bits(table0))


@pytest.mark.parametrize("tolerance", [0, 1])
@pytest.mark.parametrize("d", [3, 128])
def test_backward_ragged_bags_equal_the_mapped_and_the_expanded_apply(dev, d, tolerance):
    rows, lr = 5000, 0.05
    rng = np.random.default_rng(10 + d)
    table0 = rng.standard_normal((rows, d)).astype(np.float32)
    ids = _planted_ids(64, 26, rows, 50 + d).reshape(-1)
    n = ids.size
    off = np.concatenate([[0, 0], np.sort(rng.integers(0, n, 40)), [n, n]]).astype(np.int64)
    B = off.size - 1
    g = rng.standard_normal((B, d)).astype(np.float32)
    d_ids, d_g, d_off = torch.from_numpy(ids).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(off).to(dev)
    which = ops.bag_of(d_off, n)
    assert np.array_equal(which.cpu().numpy(), bag_model.bag_of(off, n))
    plan = ops.IndexPlan(n, dev).sort(d_ids)
    L = _lib.load()
    prev = ops.set_tolerance_mode(tolerance)
    try:
        t_bag = torch.from_numpy(table0).to(dev)
        ops.sgd_apply_bags(t_bag, plan, d_g, lr, bag_of=which)
        t_map = torch.from_numpy(table0).to(dev)
        _lib.check(L.ha_apply_mapped(ctypes.c_void_p(t_map.data_ptr()), rows, d, ctypes.c_void_p(plan.ws.data_ptr()), n,
                                     ctypes.c_void_p(d_g.data_ptr()), ctypes.c_float(lr), None,
                                     ctypes.c_void_p(which.data_ptr()), None, ops._stream_ptr()), "ha_apply_mapped")
        t_exp = torch.from_numpy(table0).to(dev)
        ops.sgd_apply(t_exp, plan, d_g[which.long()].contiguous(), lr)
        t_one = torch.from_numpy(table0).to(dev)
        ops.sgd_sparse_update_bags(t_one, d_ids, d_g, lr, offsets=d_off)
        torch.cuda.synchronize()
    finally:
        ops.set_tolerance_mode(prev)
    assert np.array_equal(_bits(t_bag), _bits(t_map))
    assert np.array_equal(_bits(t_bag), _bits(t_exp))
    assert np.array_equal(_bits(t_one), _bits(t_exp))
    if not tolerance:
        assert np.array_equal(_bits(t_bag), _bits(bag_model.sgd_bags(table0, ids, g, lr, off)))


def test_fixed_bag_apply_equals_the_mapped_apply(dev):
    """ha_apply_mapped(rowmap = NULL, valmap = bag_of, dst_init = NULL) is what ha_sgd_apply_bags(bag = F) gives."""
    B, F, d, rows, lr = 64, 26, 64, 5000, 0.05
    rng = np.random.default_rng(77)
    table0 = rng.standard_normal((rows, d)).astype(np.float32)
    ids = _planted_ids(B, F, rows, 78)
    g = rng.standard_normal((B, d)).astype(np.float32)
    d_ids, d_g = torch.from_numpy(ids).to(dev), torch.from_numpy(g).to(dev)
    plan = ops.IndexPlan(B * F, dev).sort(d_ids.reshape(-1))
    which = (torch.arange(B * F, device=dev) // F).to(torch.int32)
    t_bag = torch.from_numpy(table0).to(dev)
    ops.sgd_apply_bags(t_bag, plan, d_g, lr, bag=F)
    t_map = torch.from_numpy(table0).to(dev)
    _lib.check(_lib.load().ha_apply_mapped(ctypes.c_void_p(t_map.data_ptr()), rows, d, ctypes.c_void_p(plan.ws.data_ptr()),
                                           B * F, ctypes.c_void_p(d_g.data_ptr()), ctypes.c_float(lr), None,
                                           ctypes.c_void_p(which.data_ptr()), None, ops._stream_ptr()), "ha_apply_mapped")
    assert np.array_equal(_bits(t_bag), _bits(t_map))


# ---- operator layer ---------------------------------------------------------------------------------------------------------
def test_embedding_lookup_sum_operator_agrees_on_every_path(dev):
    """EmbeddingLookUpSum on a device table (the fused kernel) equals the PS path, the prefetched path and the cache path
    (per-occurrence rows summed in the same order) bit for bit."""
    rows, width, B, F = ROWS, 68, 9, 26
    table = _table(width)
    ids = _fixed_ids(B, F, 5)
    ids[ids >= rows] = 17                  # (the store serves valid ids)
    d_ids = torch.from_numpy(ids).to(dev)
    want = _bits(bag_model.bag_sum(table, ids))

    look = hetu_ops.EmbeddingLookUpSum(hetu_ops.EmbeddingParameter(table=torch.from_numpy(table).to(dev)))
    look.forward_hook(hetu_ops.Config(comm_mode=None, prefetch=False, use_sparse_pull=False))
    out = torch.empty((B, width), dtype=torch.float32, device=dev)
    look.compute(d_ids, out)
    assert look._fused
    assert np.array_equal(_bits(out), want)

    for name, cfg in [("ps", hetu_ops.Config(comm_mode="PS", prefetch=False)),
                      ("ps prefetched", hetu_ops.Config(comm_mode="PS", bsp=0, prefetch=True)),
                      ("cache", hetu_ops.Config(comm_mode="Hybrid", bsp=0, prefetch=False, cstable_policy="LRU",
                                                cache_bound=0, cache_limit=1000))]:
        store = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table.copy()).to(dev))
        emb = hetu_ops.EmbeddingParameter(store=store)
        comm = hetu_ops.ParameterServerCommunicateOp(emb, 0.1, next_ids=lambda: d_ids)
        comm.forward_hook(cfg, first_ids=d_ids)
        look = hetu_ops.EmbeddingLookUpSum(emb)
        look.forward_hook(cfg)
        assert not look._fused
        out = torch.full((B, width), -1.0, dtype=torch.float32, device=dev)
        look.compute(d_ids, out)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), want), name


def test_pooled_sgd_update_sparse_equals_the_expanded_one(dev):
    rows, width, B, F, lr = 5000, 36, 64, 26, 0.05
    rng = np.random.default_rng(8)
    table0 = rng.standard_normal((rows, width)).astype(np.float32)
    ids = _planted_ids(B, F, rows, 9)
    g = rng.standard_normal((B, width)).astype(np.float32)
    d_ids, d_g = torch.from_numpy(ids).to(dev), torch.from_numpy(g).to(dev)
    pooled_param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(table0).to(dev))
    grad = hetu_ops.EmbeddingLookUpSum_Gradient(pooled_param.shape).compute(d_g, d_ids)
    assert grad.pooled and grad.bag == F and grad.values.shape == (B, width)
    assert np.array_equal(_bits(grad.expanded_values()), _bits(np.repeat(g, F, axis=0)))
    hetu_ops.sgd_update_sparse(pooled_param, grad, lr)
    plain_param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(table0).to(dev))
    plain = hetu_ops.EmbeddingLookUp_Gradient(plain_param.shape).compute(d_g.repeat_interleave(F, 0).reshape(B, F, width), d_ids)
    assert not plain.pooled
    hetu_ops.sgd_update_sparse(plain_param, plain, lr)
    assert np.array_equal(_bits(pooled_param.table), _bits(plain_param.table))
    assert not np.array_equal(_bits(pooled_param.table), _bits(table0))
    # ragged bags
    off = torch.tensor([0, 0, 100, 1000, B * F], dtype=torch.int64, device=dev)
    g4 = d_g[:4].contiguous()
    ragged_param = hetu_ops.EmbeddingParameter(table=torch.from_numpy(table0).to(dev))
    rgrad = hetu_ops.EmbeddingLookUpSum_Gradient(ragged_param.shape).compute(g4, d_ids.reshape(-1), offsets=off)
    assert rgrad.pooled and rgrad.bag is None
    hetu_ops.sgd_update_sparse(ragged_param, rgrad, lr)
    want = bag_model.sgd_bags(table0, ids.reshape(-1), g[:4], lr, off.cpu().numpy())
    assert np.array_equal(_bits(ragged_param.table), _bits(want))
    # pooled slices have neither a deduplicated nor a dense form
    for fn in (grad.deduplicate, grad.to_dense, rgrad.deduplicate, rgrad.to_dense):
        with pytest.raises(ValueError):
            fn()


def test_communicate_op_pushes_pooled_slices_expanded(dev):
    """ParameterServerCommunicateOp expands pooled slices to per-occurrence values before it pushes: the store ends where the
    per-occurrence slices leave it."""
    rows, width, B, F, lr = 5000, 20, 16, 26, 0.05
    rng = np.random.default_rng(12)
    table0 = rng.standard_normal((rows, width)).astype(np.float32)
    ids = _planted_ids(64, F, rows, 13)[:B].copy()
    ids[ids >= rows] = 3
    g = rng.standard_normal((B, width)).astype(np.float32)
    d_ids = torch.from_numpy(ids).to(dev)
    tables = []
    for pooled in (True, False):
        store = ShardedEmbedding(rows, width, dev, table=torch.from_numpy(table0.copy()).to(dev))
        emb = hetu_ops.EmbeddingParameter(store=store)
        comm = hetu_ops.ParameterServerCommunicateOp(emb, lr, next_ids=lambda: d_ids)
        comm.forward_hook(hetu_ops.Config(comm_mode="PS", prefetch=False))
        d_g = torch.from_numpy(g).to(dev)
        if pooled:
            grad = hetu_ops.EmbeddingLookUpSum_Gradient(emb.shape).compute(d_g, d_ids)
        else:
            grad = hetu_ops.EmbeddingLookUp_Gradient(emb.shape).compute(d_g.repeat_interleave(F, 0).reshape(B, F, width), d_ids)
        comm.compute(grad)
        torch.cuda.synchronize()
        tables.append(_bits(store.table))
    assert np.array_equal(tables[0], tables[1])
    assert not np.array_equal(tables[0], _bits(table0))
