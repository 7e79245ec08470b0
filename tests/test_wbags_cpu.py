"""CPU-side checks of the weighted bags (the masked sum-pooled lookup of the FAE models): the six new calls are declared,
exported and bound; their arguments are validated before any device access; the numpy restatement the GPU tests are held to
(tests/wbag_model.py) agrees with tests/bag_model.py through the two identities the kernels are pinned to -- all-ones weights
give bag_sum / sgd_bags bit for bit, a 0/1 mask gives them on the compacted ragged bags -- and a dead occurrence leaves no
trace; and IndexedSlices' rules for weighted slices."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_model  # noqa: E402
import wbag_model  # noqa: E402

from herald_amd import _lib  # noqa: E402

FORWARD = ["ha_gather_wsum_f32ids", "ha_gather_wsum_u64ids"]
ONE_CALL = ["ha_sgd_sparse_update_wbags_f32ids", "ha_sgd_sparse_update_wbags_u64ids"]
SYMBOLS = FORWARD + ["ha_wbag_grad_rows", "ha_sgd_apply_wbags"] + ONE_CALL


def test_wbag_symbols_are_declared_exported_and_bound(lib):
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.ha_gather_wsum_f32ids.argtypes) == len(lib.ha_gather_wsum_u64ids.argtypes) == 11
    assert len(lib.ha_wbag_grad_rows.argtypes) == 9
    assert len(lib.ha_sgd_apply_wbags.argtypes) == 12
    assert len(lib.ha_sgd_sparse_update_wbags_f32ids.argtypes) == len(lib.ha_sgd_sparse_update_wbags_u64ids.argtypes) == 12


def test_nothing_in_the_package_imports_the_restatement():
    """The restatement is test infrastructure: nothing under herald_amd/ imports it."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "herald_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as fh:
                assert "wbag_model" not in fh.read(), name


# non-null addresses that are never dereferenced: validation comes before any device access (there is no GPU here)
P = ctypes.c_void_p(0x1000)
Q = [ctypes.c_void_p(0x2000 + 0x1000 * i) for i in range(4)]
BIG = 1 << 31

COMMON = [
    ("neither bag nor offsets", dict(bag=0, ragged=None)),
    ("both bag and offsets", dict(bag=2, ragged=P)),
    ("n not a multiple of bag", dict(n=7, bag=2, nbags=3)),
    ("n / bag is not nbags", dict(n=8, bag=2, nbags=3)),
    ("n of 2^31", dict(n=BIG, bag=2, nbags=BIG // 2)),
    ("width 0", dict(width=0)),
    ("negative width", dict(width=-4)),
    ("width of 2^30", dict(width=1 << 30)),
    ("negative n", dict(n=-1)),
    ("ragged occurrences in no bag", dict(bag=0, ragged=P, nbags=0)),
    ("null weights", dict(weights=None)),
]


@pytest.mark.parametrize("fn", FORWARD)
@pytest.mark.parametrize("case,args", COMMON + [("null table", dict(table=None)), ("null ids", dict(ids=None)),
                                                ("null out", dict(out=None))])
def test_forward_rejects_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=Q[0], rows=10, width=4, ids=P, weights=Q[1], n=8, bag=2, ragged=None, nbags=4, out=Q[2])
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["weights"], a["n"], a["bag"], a["ragged"], a["nbags"],
                          a["out"], None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("case,args", COMMON + [("null bag_grads", dict(g=None)), ("null out", dict(out=None))])
def test_grad_rows_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(g=Q[0], weights=Q[1], n=8, width=4, bag=2, ragged=None, nbags=4, out=Q[2])
    a.update(args)
    rc = lib.ha_wbag_grad_rows(a["g"], a["weights"], a["n"], a["width"], a["bag"], a["ragged"], a["nbags"], a["out"], None)
    assert rc == -1, case
    assert b"ha_wbag_grad_rows" in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("case,args", COMMON + [("null table", dict(table=None)), ("null plan_ws", dict(plan_ws=None)),
                                                ("null bag_grads", dict(g=None)),
                                                ("bag_grads aliases the table", dict(g=Q[0]))])
def test_apply_rejects_bad_arguments_before_any_device_access(lib, case, args):
    a = dict(table=Q[0], rows=10, width=4, plan_ws=P, n=8, g=Q[1], weights=Q[2], bag=2, ragged=None, nbags=4)
    a.update(args)
    rc = lib.ha_sgd_apply_wbags(a["table"], a["rows"], a["width"], a["plan_ws"], a["n"], a["g"], a["weights"], a["bag"],
                                a["ragged"], a["nbags"], 0.1, None)
    assert rc == -1, case
    assert b"ha_sgd_apply_wbags" in lib.ha_last_error(), (case, lib.ha_last_error())


@pytest.mark.parametrize("fn", ONE_CALL)
@pytest.mark.parametrize("case,args", COMMON + [("null table", dict(table=None)), ("null ids", dict(ids=None)),
                                                ("null bag_grads", dict(g=None)),
                                                ("bag_grads aliases the table", dict(g=Q[0]))])
def test_one_call_forms_reject_bad_arguments_before_any_device_access(lib, fn, case, args):
    a = dict(table=Q[0], rows=10, width=4, ids=P, weights=Q[2], n=8, g=Q[1], bag=2, ragged=None, nbags=4)
    a.update(args)
    rc = getattr(lib, fn)(a["table"], a["rows"], a["width"], a["ids"], a["weights"], a["n"], a["g"], a["bag"], a["ragged"],
                          a["nbags"], 0.1, None)
    assert rc == -1, case
    assert fn.encode() in lib.ha_last_error(), (case, lib.ha_last_error())


def test_no_ids_is_not_an_error(lib):
    for fn in FORWARD:
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, 2, None, 0, None, None) == 0
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, 0, P, 3, None, None) == 0       # ragged, every bag empty
    assert lib.ha_wbag_grad_rows(None, None, 0, 4, 2, None, 0, None, None) == 0
    assert lib.ha_wbag_grad_rows(None, None, 0, 4, 0, P, 3, None, None) == 0
    assert lib.ha_sgd_apply_wbags(None, 10, 4, None, 0, None, None, 2, None, 0, 0.1, None) == 0
    assert lib.ha_sgd_apply_wbags(None, 10, 4, None, 0, None, None, 0, P, 3, 0.1, None) == 0
    for fn in ONE_CALL:
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, None, 2, None, 0, 0.1, None) == 0
        assert getattr(lib, fn)(None, 10, 4, None, None, 0, None, 0, P, 3, 0.1, None) == 0


# ---- the restatement against tests/bag_model.py ----------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _inputs(rows, width, B, seed):
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((rows, width)) * np.exp(rng.uniform(-4, 4, (rows, 1)))).astype(np.float32)
    g = (rng.standard_normal((B, width)) * np.exp(rng.uniform(-3, 3, (B, 1)))).astype(np.float32)
    return rng, table, g


def _fixed(rng, rows, B, F):
    ids = rng.integers(0, rows, (B, F)).astype(np.float32)
    ids[:, 0] = 3                                     # one key in every bag
    ids[2, 1] = ids[2, 2] = 9                         # a duplicate inside a bag
    ids[5, 3], ids[B - 1, F - 1] = rows, rows + 7     # ids >= rows
    return ids


RAGGED = np.array([0, 0, 10, 37, 37, 37, 102, 120, 120], dtype=np.int64)


@pytest.mark.parametrize("ragged", [False, True])
def test_all_ones_weights_are_the_unweighted_bags_bit_for_bit(ragged):
    rows, width, lr = 40, 7, 0.05
    if ragged:
        rng, table, g = _inputs(rows, width, RAGGED.size - 1, 21)
        ids, off = rng.integers(0, rows + 2, 120).astype(np.float32), RAGGED
    else:
        rng, table, g = _inputs(rows, width, 33, 22)
        ids, off = _fixed(rng, rows, 33, 6), None
    w = np.ones(ids.size, dtype=np.float32)
    assert np.array_equal(_bits(wbag_model.wbag_sum(table, ids, w, off)), _bits(bag_model.bag_sum(table, ids, off)))
    got = wbag_model.wbag_sgd(table, ids, w, g, lr, off)
    assert np.array_equal(_bits(got), _bits(bag_model.sgd_bags(table, ids, g, lr, off)))
    assert not np.array_equal(_bits(got), _bits(table))


@pytest.mark.parametrize("ragged", [False, True])
def test_a_mask_is_the_unweighted_bags_on_the_compacted_ragged_bags(ragged):
    rows, width, lr = 40, 7, 0.05
    if ragged:
        rng, table, g = _inputs(rows, width, RAGGED.size - 1, 23)
        ids, off = rng.integers(0, rows + 2, 120).astype(np.float32), RAGGED
    else:
        rng, table, g = _inputs(rows, width, 33, 24)
        ids, off = _fixed(rng, rows, 33, 6), None
    w = (rng.random(ids.size) < 0.6).astype(np.float32)
    if not ragged:
        w.reshape(ids.shape)[:, 0] = 0                # the padding column
        w.reshape(ids.shape)[7, :] = 0                # a bag with no live occurrence
    w[np.flatnonzero(w == 0)[::2]] = np.float32(-0.0)
    cids, coff = wbag_model.compact(ids, w, off)
    assert 0 < cids.size < ids.size
    assert np.array_equal(_bits(wbag_model.wbag_sum(table, ids, w, off)), _bits(bag_model.bag_sum(table, cids, coff)))
    got = wbag_model.wbag_sgd(table, ids, w, g, lr, off)
    assert np.array_equal(_bits(got), _bits(bag_model.sgd_bags(table, cids, g, lr, coff)))
    assert not np.array_equal(_bits(got), _bits(table))
    # and the composed restatement: the per-occurrence gradient, then the unpooled serial apply (no -0.0 in this table)
    G = wbag_model.wbag_grad_rows(g, w, wbag_model.which_bag(ids, off))
    assert np.array_equal(_bits(G[w == 0]), np.zeros_like(_bits(G[w == 0])))
    assert np.array_equal(_bits(got), _bits(wbag_model.sgd_rows(table, ids, G, lr)))


def test_a_dead_occurrence_under_an_inf_row_or_an_inf_gradient_leaves_no_trace():
    rows, width, lr = 12, 5, 0.1
    rng, table, g = _inputs(rows, width, 4, 25)
    ids = rng.integers(1, rows, (4, 3)).astype(np.float32)
    w = rng.standard_normal((4, 3)).astype(np.float32)
    clean_sum = wbag_model.wbag_sum(table, ids, np.where(np.arange(12).reshape(4, 3) % 3 == 0, 0, w).astype(np.float32))
    ids[:, 0], w[:, 0] = 0, 0                          # the padding id, dead, in every bag
    w[2, :] = [0.0, -0.0, 0.0]                         # bag 2: no live occurrence at all
    table[0] = np.inf                                  # the padding row
    g[2] = [np.inf, -np.inf, np.nan, np.inf, np.nan]   # the gradient of the bag without live occurrences
    out = wbag_model.wbag_sum(table, ids, w)
    assert np.isfinite(out).all() and np.array_equal(_bits(out[2]), np.zeros(width, np.int32))
    assert np.array_equal(_bits(out[[0, 1, 3]]), _bits(clean_sum[[0, 1, 3]]))
    G = wbag_model.wbag_grad_rows(g, w, wbag_model.which_bag(ids))
    assert np.isfinite(G).all() and np.array_equal(_bits(G[6:9]), np.zeros((3, width), np.int32))
    got = wbag_model.wbag_sgd(table, ids, w, g, lr)
    assert np.isfinite(got[1:]).all() and np.array_equal(_bits(got[0]), _bits(table[0]))
    # a key whose only occurrences are dead keeps its bits
    only_dead = np.setdiff1d(ids[2].astype(np.int64), ids[[0, 1, 3], 1:].astype(np.int64))
    for k in only_dead:
        assert np.array_equal(_bits(got[k]), _bits(table[k]))
    # a NaN weight is not zero: the occurrence is live
    w2 = w.copy()
    w2[1, 1] = np.nan
    assert np.isnan(wbag_model.wbag_sum(table, ids, w2)[1]).all()


def test_the_sign_of_a_zero_is_the_one_corner_where_fused_and_composed_differ():
    table = np.array([[-0.0], [1.0]], dtype=np.float32)
    ids, w, g = np.array([[0.0, 1.0]], np.float32), np.array([[0.0, 1.0]], np.float32), np.array([[2.0]], np.float32)
    fused = wbag_model.wbag_sgd(table, ids, w, g, -0.5)
    G = wbag_model.wbag_grad_rows(g, w, wbag_model.which_bag(ids))
    comp = wbag_model.sgd_rows(table, ids, G, -0.5)
    assert np.signbit(fused[0, 0]) and not np.signbit(comp[0, 0]) and fused[1, 0] == comp[1, 0] == 2.0
    assert np.array_equal(_bits(wbag_model.wbag_sgd(table, ids, w, g, 0.5)), _bits(wbag_model.sgd_rows(table, ids, G, 0.5)))


# ---- IndexedSlices -----------------------------------------------------------------------------------------------------------
def test_indexed_slices_weighted_rules():
    import torch
    from herald_amd import ops
    idx, g, w = torch.zeros((2, 3)), torch.ones((2, 4)), torch.ones((2, 3))
    sl = ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag=3, weights=w)
    assert sl.weighted and sl.pooled and not sl.fm_pooled and sl.weights is w
    assert ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag_of=torch.zeros(6, dtype=torch.int32), weights=w).weighted
    assert not ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4), bag=3).weighted
    assert not ops.IndexedSlices(indices=idx, values=g, dense_shape=(10, 4)).weighted
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=g, weights=w)                                   # without bag / bag_of
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=None, bag=3, fm_grad=g, fm_sum=g, weights=w)    # not with fm_grad
    with pytest.raises(ValueError):
        ops.IndexedSlices(indices=idx, values=g, bag=3, weights=torch.ones(5))                # one weight per index
    with pytest.raises(TypeError):
        ops.IndexedSlices(indices=idx, values=g, bag=3, weights=w.double())
    with pytest.raises(ValueError, match="pooled"):
        sl.to_dense()
    # update() carries the new field, and drops it
    plain = ops.IndexedSlices()
    plain.update(idx, g, (10, 4), bag=3, weights=w)
    assert plain.weighted and plain.bag == 3
    plain.update(idx, g, (10, 4), bag=3)
    assert not plain.weighted and plain.pooled
    with pytest.raises(ValueError):
        plain.update(idx, g, (10, 4), weights=w)


def test_the_operator_pair_and_the_helper_exist():
    from herald_amd import hetu_ops, ops
    for name in ("EmbeddingLookUpWeightedSum", "EmbeddingLookUpWeightedSum_Gradient", "unweighted_slices"):
        assert hasattr(hetu_ops, name), name
    for name in ("embedding_lookup_wsum", "wbag_grad_rows", "sgd_apply_wbags", "sgd_sparse_update_wbags"):
        assert hasattr(ops, name), name
    plain = ops.IndexedSlices(indices=None, values=None)
    assert hetu_ops.unweighted_slices(plain) is plain
